/* crt_hip.h -- C ABI of the MI355X-native per-pixel hot path (libcrt_hip.so).
 *
 * This is the drop-in boundary.  The reference has no FFI; its seam is the C++ class
 * `RayTracer` (reference: SourceCode/include/tracer/RayTracer.h:96-101).  Each entry point below
 * names the reference interface it replaces.  Plain pointers and sizes only: no C++ types, no
 * torch types, no exceptions across the boundary (the reference uses assert / throw,
 * SceneParser.cpp:41,203, Vector.cpp:21-23; here every call returns an int status).
 *
 * Ownership: the caller owns every array passed in and every output buffer; the context owns its
 * device copies; no caller pointer is retained after a call returns.
 * Threading: one context = one caller thread at a time (the reference's render() is not
 * re-entrant either, RayTracer.cpp:205-213).
 * There is NO CPU fallback: without a usable HIP device crt_create fails with CRT_ERR_NO_DEVICE.
 */
#ifndef CRT_HIP_H
#define CRT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    CRT_OK = 0,
    CRT_ERR_INVALID = 1,   /* bad argument / inconsistent description */
    CRT_ERR_NO_DEVICE = 2, /* no HIP device, or the device is not usable */
    CRT_ERR_HIP = 3,       /* a HIP runtime call failed (see crt_last_error) */
    CRT_ERR_NOMEM = 4,
    CRT_ERR_IO = 5,
    CRT_ERR_PARSE = 6
};

/* Material types -- same numbering as the reference's enum MaterialType (Material.h:7). */
enum { CRT_MAT_DIFFUSE = 0, CRT_MAT_REFLECTIVE = 1, CRT_MAT_CONSTANT = 2, CRT_MAT_REFRACTIVE = 3 };
/* Texture kinds (Texture.h:24-58). */
enum { CRT_TEX_ALBEDO = 0, CRT_TEX_EDGES = 1, CRT_TEX_CHECKER = 2, CRT_TEX_BITMAP = 3 };

#define CRT_LINK_END 0xFFFFFFFFu  /* "no next node" */
#define CRT_LINK_LEAF 0x80000000u /* bit 31 of crt_node.link: the node is a leaf (unless link == CRT_LINK_END) */
#define CRT_ENTRY_LAST 0x80000000u /* bit 31 of a leaf entry: last entry of its leaf */

/* One node of the flattened ("threaded") two-level tree, 32 bytes.
 * The reference walks its KD/AABB trees with an explicit stack, pushing children[0] then
 * children[1] so that children[1] is visited first, and never prunes by distance
 * (KDTree.cpp:53-74,132-155).  The visit order is therefore a fixed property of the tree, and it
 * is encoded here as two links per node instead of a stack:
 *   box test passes, inner node : continue at `link`            (first child in visit order)
 *   box test passes, leaf       : process entries starting at (link & ~CRT_LINK_LEAF), then `miss`
 *   box test fails              : continue at `miss`            (skip the whole subtree)
 * CRT_LINK_END terminates the walk.  Nodes are stored in visit order: `link` and `miss` always point
 * to a HIGHER index (crt_create rejects anything else), so a subtree is the index range [i, miss).  Node indices are global (top-level tree and all mesh trees
 * share one array). */
typedef struct crt_node {
    float lo[3];
    uint32_t miss;
    float hi[3];
    uint32_t link;
} crt_node;

/* Triangle record used by the intersection test, 64 bytes (Ray.cpp:9-31, Triangle.cpp:37-57):
 * positions, the unit face normal (Triangle.cpp:13-16) and plane = -(v0 . normal) (Ray.cpp:17). */
typedef struct crt_triangle {
    float v0[3]; float nx;
    float v1[3]; float ny;
    float v2[3]; float nz;
    float plane; uint32_t pad[3];
} crt_triangle;

typedef struct crt_mesh {
    uint32_t root;      /* global node index of this mesh's tree root */
    uint32_t material;  /* index into materials */
    uint32_t flags;     /* bit 0: material is refractive (shadow rays skip it, AccelerationStructure.cpp:67-71) */
    uint32_t pad;
} crt_mesh;

typedef struct crt_material {
    float albedo[3];
    float ior;
    uint32_t type;    /* CRT_MAT_* */
    uint32_t smooth;  /* smooth_shading */
    int32_t texture;  /* index into textures, -1 = constant albedo */
    uint32_t pad;
} crt_material;

typedef struct crt_texture {
    uint32_t kind;      /* CRT_TEX_* */
    float color_a[3];   /* albedo | inner_color | color_A */
    float color_b[3];   /*        | edge_color  | color_B */
    float scalar;       /*        | edge_width  | square_size */
    uint32_t width, height; /* bitmap only */
    uint64_t texel_offset;  /* bitmap only: first texel in crt_scene_desc.texels */
} crt_texture;

typedef struct crt_light {
    float position[3];
    uint32_t intensity; /* unsigned, as in the reference (Scene.h:22) */
} crt_light;

/* Everything the hot path reads (the reference's `Scene` + its AccelerationStructure, flattened). */
typedef struct crt_scene_desc {
    uint32_t width, height;
    float background[3];

    const crt_node *nodes;          uint32_t n_nodes;
    uint32_t top_root;              /* node index of the top-level (object) tree root */
    const uint32_t *leaf_triangles; uint64_t n_leaf_triangles; /* mesh-tree leaf entries: global triangle index | CRT_ENTRY_LAST */
    const uint32_t *leaf_meshes;    uint32_t n_leaf_meshes;    /* top-tree leaf entries: mesh index | CRT_ENTRY_LAST */

    const crt_triangle *triangles;  uint32_t n_triangles;
    const uint32_t *triangle_vertices; /* 3 global vertex indices per triangle */
    const float *vertex_normals;    /* 3 floats per vertex (Scene.cpp:21-29) */
    const float *vertex_uvs;        /* 3 floats per vertex, may be NULL when no material has a texture */
    uint32_t n_vertices;

    const crt_mesh *meshes;         uint32_t n_meshes;
    const crt_material *materials;  uint32_t n_materials;
    const crt_texture *textures;    uint32_t n_textures;
    const uint8_t *texels;          uint64_t n_texels;  /* RGB8, 3 bytes per texel, all bitmaps concatenated */
    const crt_light *lights;        uint32_t n_lights;
} crt_scene_desc;

/* RenderOptions (RayTracer.h:25-50).  use_gi selects the reference's GI / multi-sample mode (RayTracer.cpp:90-104, 331-354):
 * RAYS_PER_PIXEL primary rays per pixel (the first through the pixel centre, the others jittered) averaged, GI_SAMPLE_SIZE
 * diffuse reflection rays at every diffuse hit, and refractive meshes no longer skipped by shadow rays
 * (AccelerationStructure.cpp:67-71).  The reference seeds that mode's generator from clock() ^ thread id (RayTracer.cpp:28-30):
 * only the distribution of its images is defined.  Here the random numbers come from a counter-based generator keyed by
 * (gi_seed, pixel, sample, position in the ray tree) -- csrc/gi_random.h -- so a frame is a function of its options, whatever
 * the device count or tile order (the GI mode's frames go through the ray-stream kernels like any other: csrc/kernel_stream.h,
 * csrc/kernel_plan.h; pixel by pixel -- csrc/kernel_lane.h -- only when level 0 does not fit 31-bit ray indices). */
typedef struct crt_options {
    uint32_t max_depth;      /* MAX_DEPTH, default 5 */
    float shadow_bias;       /* SHADOW_BIAS, default 1e-4 */
    float reflection_bias;   /* REFLECTION_BIAS */
    float refraction_bias;   /* REFRACTION_BIAS */
    uint32_t use_gi;         /* USE_GI, default 0 */
    uint32_t collect_counters; /* 1: run the counting build (every ray walked the reference's way; fills crt_stats);
                                * 2: run the production kernels and tally the tests they execute (crt_get_executed_counters) */
    uint32_t gi_sample_size; /* GI_SAMPLE_SIZE, default 2 (used when use_gi) */
    uint32_t rays_per_pixel; /* RAYS_PER_PIXEL, default 1 (used when use_gi; 0 renders like 1, as in the reference) */
    float monte_carlo_bias;  /* MONTE_CARLO_BIAS, default 1e-4 */
    uint32_t gi_seed;        /* the frame's seed of the GI generator */
} crt_options;

/* A pixel rectangle = the reference's unit of work, RayTracer::renderRectangle(row, col, w, h)
 * (RayTracer.cpp:82-112); clamped to the image like the reference does (:84-85). */
typedef struct crt_rect {
    uint32_t row, col, width, height;
} crt_rect;

/* Work counters of the last counted render: properties of (scene, camera, options) under the
 * reference's traversal semantics; they price the algorithmic bytes of SURVEY.md §8d. */
typedef struct crt_stats {
    double kernel_ms;          /* device time of the last render kernel (HIP events on the render stream) */
    double total_ms;           /* kernel + device->host copy of the last crt_render */
    uint64_t box_tests;        /* BoundingBox::hasIntersection calls */
    uint64_t tri_tests;        /* Ray::intersectWithTriangle calls */
    uint64_t leaf_index_reads; /* leaf index entries read (both tree levels) */
    uint64_t shaded_hits;      /* closest hits shaded */
    uint64_t light_evals;      /* light-loop iterations */
    uint64_t texel_fetches;    /* bitmap texel reads */
    uint64_t primary_rays, secondary_rays, shadow_rays;
    uint64_t pixels;           /* pixels rendered by the last call */
    uint32_t counters_valid;   /* 1 when the last render ran with collect_counters */
    uint32_t fallback_frames;  /* frames since crt_create whose ray queues overflowed and that were redone by the
                                * queue-less kernel (same pixels, much slower): the last resort, for a frame that outgrows
                                * queues an earlier frame of its size had fitted, and for explicit crt_tuning capacities.
                                * Updated by the synchronous calls (crt_render, crt_kernel_times_ms, crt_synchronize). */
    uint64_t queue_bytes;      /* device memory of the per-frame ray queues as allocated now (they follow the frames: they
                                * grow when a frame came close to a capacity, and after an attempt that overflowed) */
    uint64_t queue_regrows;    /* attempts since crt_create that overflowed their queues and were repeated, inside the same
                                * call, with larger ones (a context's first frame of a size is probed this way) */
} crt_stats;

typedef struct crt_ctx crt_ctx;

/* Kernel selection and sizing.  Nothing here changes a pixel: every combination renders the same frame bit for
 * bit (tests/test_gpu_parity.py runs the matrix); the defaults are what bench.py measures.  The reference has no
 * counterpart (its only tunables are RenderOptions, above); the library reads NO environment variables.
 * (Round 2's 43 fields selected between ~20 kernel variants and fed a wall-clock autotuner; the variants that lost their
 * measurements were removed -- DESIGN.md section 7 keeps the numbers, git keeps the code -- their constants are now constants,
 * and the defaults below are within 1.5 % of the best setting on every BASELINE scene.) */
enum { CRT_MODE_STREAM = 0, CRT_MODE_LANES = 1 };
typedef struct crt_tuning {
    uint32_t size;            /* sizeof(crt_tuning), filled in by crt_tuning_defaults */
    uint32_t mode;            /* CRT_MODE_STREAM (ray stream, default) | CRT_MODE_LANES (full recursion per lane, queue-less) */
    uint32_t step_budget;     /* 384: steps after which a closest-hit walk goes to the wave-per-ray kernel; 0 = faithful kernels only */
    uint32_t shadow_budget;   /* 4096: cap of the same for the bulk shadow pass (the launch scales it down with its size) */
    uint32_t level0_budget;   /* 0 (= min(step_budget, what a lane gets through in the launch)): the same for PRIMARY rays */
    uint32_t heavy_level;     /* 100000: recursion levels with fewer rays skip the per-lane kernel */
    uint32_t side_blocks;     /* 3: workgroups per CU of the bulk shadow pass on the side stream; 0 = no side stream */
    uint32_t node_cap, ray_cap, shadow_cap; /* 0 = the queues follow the frames; explicit values make
                                             * queue overflow -- and the fallback -- reachable in tests */
    uint32_t bvh;             /* 1: rays are walked through the candidate filter (csrc/crt_bvh.h, csrc/kernel_bvh.h) where the scene has one;
                               * 0: by the reference-order kernels alone; 2: the filter kernels' bounds-checked build (development) */
    uint32_t level_queue;     /* 1: with the filter kernels, every recursion level below level 0 in ONE launch that feeds itself through a queue
                               * (csrc/kernel_bvh.h: bvh_trace_queue), on this many workgroups per CU -- for frames whose levels held at most
                               * 250 k rays each a frame ago (wider levels are throughput: one launch per level is as fast or faster);
                               * 0: always one launch per level.  Development bits: 8 no child ray continues in its parent's lane; 9 the launch behind
                               * level 0 instead of beside it; 12 (tests) level 0 held back until the launch beside it has given up */
    uint32_t fetch_chunk;     /* 256 | 64 << 16: work indices a wave claims from a launch's cursor with ONE atomic -- bits 0-15 the bulk shadow
                               * pass's slots, bits 16-31 level 0's primary rays (both >= 64, multiples of 64); a cursor word serves ~100
                               * atomics per microsecond however many waves ask, which bounded the pass until it claimed in chunks */
} crt_tuning;
void crt_tuning_defaults(crt_tuning *tuning);

/* replaces RayTracer::RayTracer(Scene&) (RayTracer.cpp:45-51): copies the flattened scene + tree to
 * HBM on `device` and allocates the persistent H*W colour buffer (zero-initialised like
 * colorBuffer, RayTracer.h:69). */
int crt_create(const crt_scene_desc *scene, int device, crt_ctx **out);
/* the same with explicit tuning (NULL = defaults) */
int crt_create_tuned(const crt_scene_desc *scene, int device, const crt_tuning *tuning, crt_ctx **out);

/* replaces RayTracer::setCamera() (RayTracer.cpp:57-59): position + row-major 3x3 matrix
 * (Camera.h:7-8).  The tree is not rebuilt. */
int crt_set_camera(crt_ctx *ctx, const float position[3], const float matrix[9]);

/* replaces RayTracer::render's bucket scheduling + renderRectangle (RayTracer.cpp:141-158,82-112):
 * renders the pixels covered by `rects` into the context's persistent colour buffer (pixels not
 * covered keep their previous value) and copies the whole H*W*3 float buffer (row 0 = top) to
 * `out_rgb` (host memory, may be NULL to skip the copy). */
int crt_render(crt_ctx *ctx, const crt_options *options, const crt_rect *rects, uint32_t n_rects, float *out_rgb);

/* The same without waiting for the device: the frame (and the copies to out_rgb -- float, H*W*3 -- and / or out_rgb8 --
 * quantised bytes, PPMColor rule; either may be NULL; pinned host memory keeps the copies asynchronous) is enqueued and the
 * call returns.  crt_wait finishes it and fills the statistics.  One frame per context at a time: a second crt_render_async
 * first waits for the previous frame.  Frames IN FLIGHT together need one context each (the reference's animation driver,
 * app/animation.cpp:24-38, renders frame after frame; crt::RayTracer::renderAsync alternates two contexts).
 * THE FIRST FRAME OF A SIZE / DEPTH ON A CONTEXT IS NOT ASYNCHRONOUS: its queue capacities are probed -- the call waits for the
 * attempt (hipEventSynchronize on the frame's stream) and repeats it with larger queues if it overflowed (crt_stats::queue_regrows) --
 * and so is the frame after one that overflowed.  That also holds for crt_render_tiles_device on a caller's stream: such a call
 * cannot be captured into a hipGraph; render one frame first, capture the following ones.  The library also uses two streams of its
 * own beside the caller's (the bulk shadow pass; the level queue's launch), joined to it by events before the call's last launch. */
int crt_render_async(crt_ctx *ctx, const crt_options *options, const crt_rect *rects, uint32_t n_rects, float *out_rgb,
                     uint8_t *out_rgb8);
int crt_wait(crt_ctx *ctx);
/* page-locked host memory for those outputs (NULL when it cannot be had) */
void *crt_alloc_pinned(size_t bytes);
void crt_free_pinned(void *p);

/* Device-resident variants used by the multi-GPU tile partition.
 * The frame is cut into 8x8 pixel tiles, numbered row-major; this call renders tiles
 * first, first+stride, first+2*stride, ... and writes them PACKED, tile after tile, 64 pixels x 3
 * floats each (pixel k of a tile = row k/8, column k%8), to `d_packed` (device memory of at least
 * crt_packed_tile_count(...)*192 floats).  Asynchronous on `stream` (a hipStream_t, NULL = default). */
int crt_render_tiles_device(crt_ctx *ctx, const crt_options *options, uint32_t first, uint32_t stride,
                            float *d_packed, void *stream);
/* number of tiles the call above renders */
uint32_t crt_packed_tile_count(const crt_ctx *ctx, uint32_t first, uint32_t stride);
/* Scatter `n_parts` packed buffers (part p holds tiles p, p+n_parts, ...; laid out one after another in
 * d_packed_all with `part_stride_floats` between parts) into the row-major H*W*3 device frame d_frame. */
int crt_unpack_tiles_device(crt_ctx *ctx, const float *d_packed_all, uint32_t n_parts, uint64_t part_stride_floats,
                            float *d_frame, void *stream);

/* PPMColor quantiser (Color.cpp:12-16) on the device: out[i] = (uint8)(clamp(rgb[i],0,1)*255), truncating. */
int crt_quantize_device(crt_ctx *ctx, const float *d_rgb, uint64_t n_values, uint8_t *d_out, void *stream);
/* Quantised copy of the context's persistent colour buffer to host memory (H*W*3 bytes). */
int crt_read_quantized(crt_ctx *ctx, uint8_t *out_rgb8);

/* Device time of the most recent render kernel, from the HIP events recorded around it on the stream
 * it was launched on (waits for that kernel to finish). */
int crt_kernel_elapsed_ms(crt_ctx *ctx, double *ms);
/* Device times of the most recent renders (up to 64, oldest first), from HIP events recorded around the
 * kernels on the streams they were launched on; 5 doubles per render:
 *   [0] whole render, first kernel to last
 *   [1] the recursion levels: stream_trace_shade + heavy_trace_closest + stream_shade_evicted, all levels
 *   [2] stream_trace_shadow pass 0 (level-0 shadow rays; runs on a side stream BESIDE [1])
 *   [3] stream_trace_shadow pass 1 + heavy_trace_shadow   [4] stream_resolve (+ fallback)
 * Waits for those kernels to finish. */
int crt_kernel_times_ms(crt_ctx *ctx, double *out_phase_ms, uint32_t max_count, uint32_t *count);
int crt_get_stats(crt_ctx *ctx, crt_stats *out);
/* The counters of the last counted render split by kernel, in crt_stats order: box_tests, tri_tests,
 * leaf_index_reads, shaded_hits, light_evals, texel_fetches, primary_rays, secondary_rays, shadow_rays.
 * closest = stream_trace_shade of all recursion levels, shadow = stream_trace_shadow pass 0 (the level-0 shadow
 * rays); shadow pass 1 and the resolve are only in crt_stats' totals. */
int crt_get_kernel_counters(crt_ctx *ctx, uint64_t closest[9], uint64_t shadow[9]);
int crt_synchronize(crt_ctx *ctx);
void crt_destroy(crt_ctx *ctx);
/* last error text of a context (or of the last failed crt_create when ctx == NULL) */
const char *crt_last_error(const crt_ctx *ctx);
int crt_device_count(void);

/* ---- Ray queries: closest hit and occlusion for rays the CALLER supplies -- picking, visibility and ambient-occlusion baking
 * between arbitrary points, a depth / normal / object-id pass.  The reference has these two operations as its seam below shootRay:
 * AccelerationStructure::intersect (KDTree.cpp:127-192) and AccelerationStructure::checkForIntersection
 * (AccelerationStructure.cpp:56-94).  Kernels: csrc/kernel_query.h.  Single-device contexts only (not crt_multi).
 *
 * crt_trace_rays* returns what AccelerationStructure::intersect returns for Ray{origin, direction, ray_type}: the same winner under
 *   the reference's collection order (the first collected hit, replaced only by a strictly smaller distance, at both tree levels:
 *   KDTree.cpp:75-86, 156-167), the same t and point float for float (Ray.cpp:19-23), the face normal or -- for a smooth material --
 *   the interpolated, normalised one (KDTree.cpp:180-185), (u, v) as Triangle::getBarycentricCoordinates gives them
 *   (Triangle.cpp:63-73; computed for smooth or textured materials only, otherwise 0).  A winner with t = +inf or NaN (a ray parallel
 *   to a triangle's plane, Ray.cpp:19) is a hit and is reported as one.  ray_type matters the way it does in the reference:
 *   CRT_RAY_PRIMARY culls back faces (Ray.cpp:13), the other three behave alike.
 * crt_occluded_rays* returns checkForIntersection(ray, max_distance[i]) of the non-GI build for a shadow ray
 *   (AccelerationStructure.cpp:56-94): refractive meshes are skipped (:67-71), a mesh occludes when its closest hit lies within
 *   length(point - origin) <= max_distance (:73-74).  max_distance may be +inf.  (The GI build's rule -- no mesh is skipped -- is not
 *   offered.)  The radiance queries of the GI mode, crt_shoot_rays_gi* below, light their records by that rule.
 * Directions are used AS GIVEN, like the reference's Ray holds them (Ray.h): nothing is normalised (RayTracer::getRay and shootRay
 *   normalise before they build a Ray, RayTracer.cpp:78,420, and so do callers who want that).  The candidate filter's error analysis
 *   (csrc/kernel_bvh.h) takes |d| = 1 up to rounding, so a ray with | dx^2 + dy^2 + dz^2 - 1 | > 2^-20 (evaluated in float32; every
 *   float32-rounded unit vector is within 2^-21: csrc/kernel_query.h, QUERY_UNIT_TOL) or with a non-finite coordinate is answered by
 *   the reference-order walk instead.  The answer is exact for EVERY ray; only the speed differs.
 * n == 0 is CRT_OK and touches nothing; a NULL array with n > 0 or an unknown ray_type is CRT_ERR_INVALID.  Any n that fits the
 *   arrays works.  The host variants copy in, run, copy out and return when the result is in `out`.  The device variants are
 *   asynchronous on `stream` (a hipStream_t, NULL = default) and allocate nothing after the first call of a given size (the scratch
 *   is the context's: a call on ANOTHER stream than the previous query's first waits for that one).  A query on a context with a
 *   crt_render_async frame pending first waits for it, as a second crt_render_async does.  A query leaves the persistent colour
 *   buffer, crt_stats, the ray queues' sizing and fallback_frames exactly as they were. */
enum { CRT_RAY_PRIMARY = 0, CRT_RAY_SHADOW = 1, CRT_RAY_REFLECTION = 2, CRT_RAY_REFRACTION = 3 };   /* enum RayType, Ray.h:14 */
typedef struct crt_ray { float origin[3]; float direction[3]; } crt_ray;   /* 24 bytes: Ray's origin and direction (Ray.h) */
/* Intersection (KDTree.cpp:168-190), 48 bytes */
typedef struct crt_hit {
    float t; float point[3]; float normal[3]; float u, v;
    uint32_t mesh, triangle;   /* triangle: index into crt_scene_desc.triangles (global) */
    uint32_t hit;              /* 0: the reference reports no intersection; every other field is then 0 */
} crt_hit;
typedef struct crt_query_stats {
    uint64_t rays;             /* rays of the last query call */
    uint64_t hits;             /* ... with a hit / occluded */
    uint64_t rerouted;         /* ... answered by the reference-order walk: direction not of unit length, non-finite ray, a miss
                                * refuted by the miss check, filter stack exhausted; all of them when the scene has no filter or
                                * crt_tuning::bvh == 0 */
    double kernel_ms;          /* device time of its launches (HIP events on its stream) */
} crt_query_stats;
int crt_trace_rays(crt_ctx *ctx, const crt_ray *rays, uint64_t n, uint32_t ray_type, crt_hit *out);
int crt_trace_rays_device(crt_ctx *ctx, const crt_ray *d_rays, uint64_t n, uint32_t ray_type, crt_hit *d_out, void *stream);
int crt_occluded_rays(crt_ctx *ctx, const crt_ray *rays, const float *max_distance, uint64_t n, uint8_t *out);
int crt_occluded_rays_device(crt_ctx *ctx, const crt_ray *d_rays, const float *d_max_distance, uint64_t n, uint8_t *d_out, void *stream);
/* RayTracer::getRay (RayTracer.cpp:61-80) at the centre of every pixel with the camera of crt_set_camera: H*W rays, row-major, to
 * device memory; asynchronous on `stream`.  The direction is normalised once, as getRay returns it. */
int crt_camera_rays_device(crt_ctx *ctx, crt_ray *d_rays, void *stream);
/* statistics of the last query call (ray query or direct-lighting query); waits for it */
int crt_get_query_stats(crt_ctx *ctx, crt_query_stats *out);

/* ---- Direct lighting for hit records and points the CALLER supplies -- light baking (lightmap texels, per-vertex lighting), the colour
 * under a picked ray, a direct-light pass over a ray set of the caller's.  The reference's one non-recursive stage below shootRay:
 * RayTracer::calculateDiffusion of the non-GI build (RayTracer.cpp:300-330).  Kernels: csrc/kernel_shade.h.  Single-device contexts only.
 *
 * crt_shade_hits* returns, for record i, the colour shootRay returns for a ray whose intersect() result is hits[i] (e.g. what
 *   crt_trace_rays* wrote), wherever shootRay does not recurse, and says which case it was in out_status[i] (may be NULL):
 *   CRT_SHADE_BACKGROUND  hit == 0 (RayTracer.cpp:449-450) or the mesh's material is constant (:443-446): the scene's background;
 *   CRT_SHADE_DIFFUSE     calculateDiffusion: for every light in scene order the shadow ray from point + normal * shadow_bias towards
 *                         it, checkForIntersection(shadowRay, distanceToLight) (refractive meshes skipped), and where it is unoccluded
 *                         colour = colour + intensity / (4 r^2 pi) * max(0, l . n) * base; base = the material's albedo or
 *                         Texture::getColor at the record's (u, v, 1 - u - v) and triangle.  The same float for float, NaNs included: a
 *                         record with a non-finite point (a hit at t = inf) is shaded the way the reference shades it;
 *   CRT_SHADE_RECURSES    a reflective or refractive material: shootRay would shoot further rays, which is not offered HERE (the radiance
 *                         queries below, crt_shoot_rays*, follow them); colour 0, 0, 0;
 *   CRT_SHADE_INVALID     hit != 0 with mesh >= n_meshes or triangle >= n_triangles; colour 0, 0, 0.  Both indices are compared with
 *                         the scene's counts before anything is read through them; whether the triangle BELONGS to the mesh is not
 *                         checked (in-range indices are safe to read; the colour is then that mix's).
 *   Of `options` only shadow_bias is read; use_gi != 0 is CRT_ERR_INVALID (the GI build's occlusion rule -- no mesh skipped -- and its
 *   division by GI_SAMPLE_SIZE + 1 are not offered).  A GI record's whole colour is crt_shoot_rays_gi*'s, below.
 * crt_light_points* returns out[i] = the sum, in light order, of the unoccluded lights' factors intensity / (4 r^2 pi) * max(0, l . n) at
 *   points[i] with normals[i] (3 floats each): calculateDiffusion's result for a white (1, 1, 1) untextured diffuse surface, channel
 *   for channel.
 * A scene without lights gives 0.  n == 0 is CRT_OK and touches nothing; a NULL required array (or options) with n > 0 is
 *   CRT_ERR_INVALID.  Host and device variants, streams, the pending frame, what is left alone: as for the ray queries above, whose
 *   scratch these calls share.  crt_get_query_stats: rays = n, hits = records shaded DIFFUSE (crt_light_points: n), rerouted = records
 *   whose lights were all redone by the reference-order walk -- a shadow ray with a non-finite coordinate or a zero direction (a light
 *   AT the point), filter stack exhausted; every DIFFUSE record when the scene has no filter or crt_tuning::bvh == 0. */
enum { CRT_SHADE_BACKGROUND = 0, CRT_SHADE_DIFFUSE = 1, CRT_SHADE_RECURSES = 2, CRT_SHADE_INVALID = 3 };
int crt_shade_hits(crt_ctx *ctx, const crt_hit *hits, uint64_t n, const crt_options *options, float *out_rgb, uint8_t *out_status);
int crt_shade_hits_device(crt_ctx *ctx, const crt_hit *d_hits, uint64_t n, const crt_options *options, float *d_rgb, uint8_t *d_status,
                          void *stream);
int crt_light_points(crt_ctx *ctx, const float *points, const float *normals, uint64_t n, float shadow_bias, float *out);
int crt_light_points_device(crt_ctx *ctx, const float *d_points, const float *d_normals, uint64_t n, float shadow_bias, float *d_out,
                            void *stream);

/* ---- Radiance queries: the colour RayTracer::shootRay returns for rays the CALLER supplies, with its reflections, refractions and
 * Fresnel mix -- fisheye, panoramic and stereo cameras, light probes and cube maps from arbitrary points, depth of field, the colour
 * under a picked ray, re-shooting only a frame's changed pixels.  Kernels: csrc/kernel_radiance.h around those of the two query families
 * above.  Single-device contexts only.
 *
 * out_rgb[3 i ..] is what shootRay(Ray{origin, direction, ray_type}, depth = 0) of the non-GI build returns (RayTracer.cpp:419-451):
 *   the direction NORMALISED ON ENTRY, as shootRay does it (:420; a zero direction stays zero) -- unlike crt_trace_rays*, which walks
 *   directions as given --, then the closest hit, the switch on the material, calculateDiffusion, calculateReflection,
 *   calculateRefraction (the Fresnel term through the restated glibc powf) and the depth rule: a ray that would enter shootRay with
 *   depth > max_depth is the background.  The same float for float, NaNs included.  ray_type is the caller's ray's alone
 *   (CRT_RAY_PRIMARY culls back faces); its children are REFLECTION and REFRACTION rays, as in the reference.  A frame is the special
 *   case of crt_camera_rays_device's rays as CRT_RAY_PRIMARY: getRay's normalisation followed by shootRay's is the frame's ray.
 * Of `options` max_depth, shadow_bias, reflection_bias and refraction_bias are read.  use_gi != 0, max_depth + 1 > 64 (a frame's rule),
 *   an unknown ray_type, a NULL array or NULL options with n > 0 are CRT_ERR_INVALID; n == 0 is CRT_OK and touches nothing.  The GI
 *   mode's colours are crt_shoot_rays_gi*'s, below.
 * The evaluation is LEVEL-SYNCHRONOUS: for recursion level g = 0 .. max_depth the level's rays are traced (crt_trace_rays*' kernels) and
 *   lit (crt_shade_hits*' kernels), the mirror and glass hits' child rays become level g + 1, and when no level is left the colours are
 *   mixed from the deepest level up.  Every level has arrays of its own in the context's scratch, which grows and is kept: a call
 *   allocates nothing once the context has seen a call whose levels were at least as wide.
 * The device variant takes device pointers and enqueues on `stream`, BUT IT WAITS FOR THE STREAM ONCE PER LEVEL (and once per 2^22 rays
 *   of n): the size of level g + 1 -- one 4-byte count -- is read back through pinned memory before that level can be launched.  Such a call
 *   therefore CANNOT BE CAPTURED INTO A hipGraph, and it returns when its last level's launches are enqueued, not before.  The host
 *   variant copies in, runs, copies out and returns when the colours are in out_rgb.
 * The pending frame, what is left alone (the persistent colour buffer, crt_stats, the ray queues' sizing, fallback_frames), streams: as
 *   for the ray queries.  crt_get_query_stats after a call: rays = n, hits = the callers' rays with a hit (level 0), rerouted and
 *   kernel_ms as in crt_shoot_stats.  A query call after a radiance call first waits for it. */
typedef struct crt_shoot_stats {
    uint64_t rays;             /* n */
    uint32_t levels;           /* recursion levels that held at least one ray */
    uint32_t pad;
    uint64_t level_rays[64];   /* rays traced at level g (MAX_GENERATIONS entries) */
    uint64_t shadow_records;   /* DIFFUSE nodes over all levels: records whose lights were walked */
    uint64_t rerouted;         /* sum of the constituent queries' rerouted counts (crt_query_stats::rerouted of every level's trace and
                                * lighting launches) */
    double kernel_ms;          /* HIP events on the call's stream, first launch to last: the waits between the levels are inside */
} crt_shoot_stats;
int crt_shoot_rays(crt_ctx *ctx, const crt_ray *rays, uint64_t n, uint32_t ray_type, const crt_options *options, float *out_rgb);
int crt_shoot_rays_device(crt_ctx *ctx, const crt_ray *d_rays, uint64_t n, uint32_t ray_type, const crt_options *options, float *d_rgb,
                          void *stream);
/* statistics of the last radiance call; waits for it */
int crt_get_shoot_stats(crt_ctx *ctx, crt_shoot_stats *out);

/* ---- Radiance queries in the GI / multi-sample mode (crt_options::use_gi) -- light probes and irradiance volumes, lightmap texels with
 * bounce light, a fisheye, panoramic or stereo camera in the GI mode, re-shooting a GI frame's changed pixels.  Kernels: the GI builds of
 * csrc/kernel_radiance.h.  Single-device contexts only.
 *
 * out_rgb[3 i ..] is what shootRay(Ray{origin, direction, ray_type}, depth = 0) of the GI build returns (RayTracer.cpp:419-451, 300-356),
 *   with the counter-based generator of csrc/gi_random.h in place of the reference's clock-seeded one, the invocation's key being keys[i]:
 *   a key is a ray's place in a ray tree.  keys == NULL means keys[i] = crt_gi_mix(crt_gi_mix(options->gi_seed, (uint32_t)i), 0), the key
 *   of a frame's pixel i, sample 0: the camera's rays (crt_camera_rays_device) shot as CRT_RAY_PRIMARY are then the GI frame of that seed
 *   with rays_per_pixel = 1, up to the frame's `0 + colour` (a -0 channel is +0 there).  A colour is a function of (scene, ray, key,
 *   options) alone: not of n, of the ray's position in the array, of how the call is split into passes, or of the device.
 * What the GI build changes (the rest is crt_shoot_rays*'s arithmetic):
 *   * shadow rays skip no mesh (AccelerationStructure.cpp:67-71);
 *   * a DIFFUSE hit, after its direct light, shoots gi_sample_size rays from point + normal * monte_carlo_bias, sample i in the direction
 *     the reference forms from the incoming direction, the normal and the key's numbers u(key, 2 + 2 i), u(key, 3 + 2 i) (RayTracer.cpp:
 *     333-347), as a REFLECTION ray with key crt_gi_child_key(key, 2 + i) entering shootRay at depth + 1, and returns
 *     (direct + (((0 + c_0) + c_1) + ...)) * (1 / (float)(gi_sample_size + 1)); a sample that would enter beyond max_depth is the
 *     background, added without tracing; no samples: (direct + 0) * (1 / 1);
 *   * a mirror's or glass hit's children carry the keys crt_gi_child_key(key, 0) and (key, 1).
 * Of `options` max_depth, shadow_bias, reflection_bias, refraction_bias, monte_carlo_bias and gi_sample_size are read, gi_seed when keys
 *   is NULL.  rays_per_pixel is NOT read: averaging a pixel's samples is the caller's -- as the reference does it (RayTracer.cpp:90-104;
 *   oracle/cpu_ref.c: render_pixel): sample s of pixel p has the key crt_gi_mix(crt_gi_mix(seed, p), s), the sum starts at 0 and takes the
 *   samples in order from 0, times 1 / (float)n.
 * CRT_ERR_INVALID: use_gi == 0 (those colours are crt_shoot_rays*'s), gi_sample_size > 64 (a frame's rule), max_depth + 1 > 64, an unknown
 *   ray_type, NULL rays, options or output with n > 0 -- and a call whose levels could not be held: level g + 1 is up to
 *   max(2, gi_sample_size) times as wide as level g, so a call is evaluated in passes of
 *   clamp(2^26 / max(2, gi_sample_size)^max_depth, 64, 2^22) rays, which keeps the deepest level of a pass at 2^26 rays in the worst case
 *   (about 8 GB of level arrays; what a scene needs is allocated, not the worst case); when not even 64 rays fit, the call is refused
 *   before anything runs.  n == 0 is CRT_OK and touches nothing.
 * Everything else is crt_shoot_rays*'s contract, above: the direction normalised on entry, the level-synchronous evaluation (a DIFFUSE
 *   record is a node here too, its samples gi_sample_size consecutive rays of the next level), host and device variants, streams, the
 *   pending frame, what is left alone, the device variant's ONE WAIT PER LEVEL and pass -- it cannot be captured into a hipGraph --,
 *   crt_get_shoot_stats (level_rays, shadow_records, rerouted, kernel_ms) and crt_get_query_stats. */
int crt_shoot_rays_gi(crt_ctx *ctx, const crt_ray *rays, const uint32_t *keys, uint64_t n, uint32_t ray_type,
                      const crt_options *options, float *out_rgb);
int crt_shoot_rays_gi_device(crt_ctx *ctx, const crt_ray *d_rays, const uint32_t *d_keys, uint64_t n, uint32_t ray_type,
                             const crt_options *options, float *d_rgb, void *stream);

/* ---- Radiance queries with no host wait: crt_shoot_rays_device's and crt_shoot_rays_gi_device's colours from a call that only ENQUEUES
 * and can be captured into a hipGraph -- light probes re-shot every frame, other cameras, depth of field, re-shooting changed pixels
 * inside an animation loop.  Kernels: the DEVN builds of csrc/kernel_query.h, kernel_shade.h and kernel_radiance.h.  Single-device
 * contexts only.
 *
 * The colours are crt_shoot_rays_device's (crt_shoot_rays_gi_device's), bit for bit, for every ray whose ray tree lost no child (below).
 *   The walks, the lighting, the scatter and combine arithmetic, the keys and ray_type are those calls'; the same `options` fields are
 *   read and the same CRT_ERR_INVALID rules hold for use_gi, gi_sample_size, max_depth, ray_type and NULL arguments.  n == 0 is CRT_OK and
 *   touches nothing.  A call is ONE pass: n > 2^22 is CRT_ERR_INVALID, the caller splits.  The GI calls' worst-case product rule (64 x
 *   fan^max_depth <= 2^26) does not apply: the capacities bound the memory.
 * Level capacities.  With fan = 2 (the GI call: max(2, gi_sample_size)), level g, 1 <= g <= max_depth, holds at most
 *   min(level_cap[g], fan^g n, 2^30) rays (the GI call: and (2^32 - 1) / fan while g < max_depth, so that no 32-bit count wraps);
 *   level_cap has max_depth + 1 entries and level_cap[0] is ignored.  level_cap == NULL means "what this context's level arrays hold now":
 *   the width earlier radiance calls left (the scratch grows and is kept, and those calls reserve fan x a level's rays for the level
 *   below it).  The intended use is the frames' pattern: one ordinary crt_shoot_rays_device call to size the context, then enqueue calls.
 *   With explicit capacities, and outside a capture, the call first grows the scratch to them, like any other query.
 * No waits.  The call enqueues its launches on `stream` and returns: no hipStreamSynchronize, no readback that the host waits for.  Every
 *   level's kernels are launched for the level's CAPACITY and read the level's actual size from a device word (the count of the rays
 *   appended to it, clamped to the capacity).  A level that ran dry costs empty launches, nothing else.
 * Overflow.  A child that does not fit its level becomes the background, as a child beyond max_depth is; nothing is written out of
 *   bounds, the return code stays CRT_OK, and the report says so (overflow, dropped).  Colours of rays whose ray tree lost no child are
 *   still exact; the caller repeats the call with larger capacities, or uses the synchronous call.  (GI: a DIFFUSE record's samples fit
 *   as a block or not at all; slots of the level that a refused block leaves unwritten are traced with what they held, and count in
 *   level_rays, not in dropped.  No other ray reads their colours.)
 * d_report (device memory, 8-byte aligned; may be NULL) is filled by one small kernel behind the last launch.
 * Outside a capture the call is an open call like the other device calls: events are recorded around it, crt_get_shoot_stats and
 *   crt_get_query_stats are filled from the report (copied to pinned memory behind the last launch) and crt_get_shoot_report returns
 *   it.  The waiting rules of the other queries apply (a pending crt_render_async frame, an open call on another stream, an open call
 *   of another kind are waited for first), with one exception: an enqueue call behind an enqueue call on the SAME stream waits for
 *   nothing and supersedes its statistics.
 * While `stream` is being captured (hipStreamIsCapturing) the call makes NO HIP call that synchronises, allocates or records one of the
 *   library's events.  If it would need one -- a pending crt_render_async frame, an open call to harvest, scratch that would have to
 *   grow (a context without a radiance call so far has none) -- it returns CRT_ERR_INVALID with a message that names the reason BEFORE
 *   it enqueues anything, so the capture stays valid.  It leaves no open call behind and touches no statistics: those of the replays
 *   come through d_report alone.
 * The captured graph is a single chain on the caller's stream -- no second stream, no parallel branch.  It holds pointers into the
 *   context's scratch: it is valid while crt_query_scratch_generation(ctx) is unchanged and the context lives.  While it may be running,
 *   ordering other queries of this context behind it is the caller's job (they share the scratch). */
typedef struct crt_shoot_report {   /* written by the DEVICE, 8-byte aligned */
    uint32_t levels;           /* recursion levels that held at least one ray */
    uint32_t overflow;         /* 0, or 1 + the first level g whose children did not all fit level g + 1 */
    uint64_t dropped;          /* children that did not fit, all levels */
    uint64_t level_rays[64];   /* rays traced at level g */
    uint64_t hits;             /* the caller's rays with a hit (level 0) */
    uint64_t shadow_records, rerouted;   /* as in crt_shoot_stats */
} crt_shoot_report;
int crt_shoot_rays_enqueue(crt_ctx *ctx, const crt_ray *d_rays, uint64_t n, uint32_t ray_type, const crt_options *options, float *d_rgb,
                           const uint32_t *level_cap, crt_shoot_report *d_report, void *stream);
int crt_shoot_rays_gi_enqueue(crt_ctx *ctx, const crt_ray *d_rays, const uint32_t *d_keys, uint64_t n, uint32_t ray_type,
                              const crt_options *options, float *d_rgb, const uint32_t *level_cap, crt_shoot_report *d_report, void *stream);
/* host copy of the last non-captured enqueue call's report; waits for it */
int crt_get_shoot_report(crt_ctx *ctx, crt_shoot_report *out);
/* changes whenever any query scratch array is reallocated */
uint64_t crt_query_scratch_generation(const crt_ctx *ctx);

/* ---- Progressive GI frames: a frame with rays_per_pixel = R rendered sample pass by sample pass, in memory that does not depend on R,
 * displayable after every pass, continuable, and THE ONE-SHOT FRAME BIT FOR BIT when the last pass is in.  Kernels: csrc/kernel_progressive.h
 * around the GI radiance queries'.  Single-device contexts only.  No frame kernel is involved.
 *
 * The fold.  A GI frame's rule for pixel p is a plain left fold (RayTracer.cpp:90-104; oracle/cpu_ref.c: render_pixel): sum = 0;
 *   sum = sum + c_s for s = 0 .. n - 1, where c_s is shootRay's colour for the ray of sample s under the key
 *   crt_gi_mix(crt_gi_mix(gi_seed, p), s); sample 0 goes through the pixel centre, the others through (px + u(key, 0), py + u(key, 1));
 *   the pixel is sum * (1 / (float)n).  A colour is a function of (scene, ray, key, options) alone, so the fold can be cut anywhere:
 *   after samples 0 .. k in order, the mean below is the GI frame with rays_per_pixel = k + 1 -- the same floats, `0 + c_0` included.
 * crt_camera_sample_rays_device: for i < n, pixel p = d_pixels ? d_pixels[i] : i (row-major); d_keys[i] = crt_gi_mix(crt_gi_mix(gi_seed,
 *   p), sample) (d_keys may be NULL); d_rays[i] = RayTracer::getRay for that pixel with the camera of crt_set_camera: sample == 0 the
 *   pixel centre -- crt_camera_rays_device's bits --, otherwise the jittered position above, the direction normalised ONCE, as getRay
 *   returns it (crt_shoot_rays_gi* does shootRay's own normalisation on entry).  With d_pixels == NULL, n must be width * height:
 *   anything else is CRT_ERR_INVALID.  With a list, an index >= width * height gives a ray with zero direction and key 0, and nothing
 *   is read through that index.
 * crt_accumulate_samples_device: for i < n and pixel p as above (the same rule for a NULL list), channel by channel
 *   d_sum[3p + c] = (sample == 0 ? 0.0f : d_sum[3p + c]) + d_rgb[3i + c], and where d_mean != NULL
 *   d_mean[3p + c] = d_sum[3p + c] * (1.0f / (float)(sample + 1)).  d_sum and d_mean are width * height * 3 floats of the caller's; an
 *   out-of-range p is skipped.  THE PIXELS OF ONE CALL MUST BE DISTINCT: a pixel listed twice is two threads on one sum, the caller's
 *   race.  Samples must arrive in order from 0 for the mean to be the frame's.
 * Both only ENQUEUE on `stream` (a hipStream_t, NULL = default): no wait, no allocation, no readback, so they can be captured into a
 *   hipGraph like crt_shoot_rays_gi_enqueue, with which they compose: rays and keys of a sample -> colours -> fold, on one stream.
 *   Pixel lists give adaptive sampling to a caller who wants it.
 * crt_render_progressive: samples first_sample .. first_sample + n_samples - 1 of EVERY pixel of the frame (render()'s bucket grid can
 *   leave edge rows of a frame unrendered; this call has no grid), shot through crt_shoot_rays_gi_device's path in its usual passes --
 *   the level arrays are bounded by one pass whatever the sample count --, one sample at a time and in order, and folded into a
 *   context-owned width * height * 3 sum (allocated on first use, freed by crt_destroy).  The mean goes to the context's persistent colour
 *   buffer, so crt_read_quantized works unchanged, and to out_rgb (host memory, may be NULL); the call returns when it is there.
 *   Of `options` the fields crt_shoot_rays_gi* reads are read, and gi_seed; rays_per_pixel is NOT read.
 *   first_sample == 0 starts a new frame, whatever the context holds.  CRT_ERR_INVALID, with nothing changed: any other
 *   first_sample != crt_progressive_samples(ctx);
 *   use_gi == 0; whatever the GI radiance calls refuse (gi_sample_size > 64, max_depth + 1 > 64, levels that cannot be held, NULL options).
 *   n_samples == 0 is CRT_OK and touches nothing.  crt_set_camera and crt_render* reset crt_progressive_samples to 0.
 *   The call waits for a pending crt_render_async frame, as the queries do; it leaves crt_stats, the ray queues' sizing and
 *   fallback_frames as they were; crt_get_shoot_stats describes the last sample.  Behind a frame's sample 0 the level arrays are given a
 *   quarter of headroom, so that later samples -- whose levels differ by the pixels whose jittered ray meets another material -- do not
 *   regrow them (crt_query_scratch_generation tells when one did). */
int crt_camera_sample_rays_device(crt_ctx *ctx, uint32_t gi_seed, uint32_t sample, const uint32_t *d_pixels, uint64_t n, crt_ray *d_rays,
                                  uint32_t *d_keys, void *stream);
int crt_accumulate_samples_device(crt_ctx *ctx, const float *d_rgb, const uint32_t *d_pixels, uint64_t n, uint32_t sample, float *d_sum,
                                  float *d_mean, void *stream);
int crt_render_progressive(crt_ctx *ctx, const crt_options *options, uint32_t first_sample, uint32_t n_samples, float *out_rgb);
/* samples folded into the context's sum so far */
uint32_t crt_progressive_samples(const crt_ctx *ctx);

/* ---- Adaptive sampling for progressive GI frames: a pixel whose samples agree stops being shot.  A per-pixel noise estimate, a stopping
 * rule and a device-side compaction of "which pixels go on" into the next pass's pixel list, beside the two primitives above.  Kernels:
 * csrc/kernel_adaptive.h; the rule, one header for host and device: csrc/adaptive_rule.h.  A pixel that stopped after k samples is the
 * one-shot GI frame with rays_per_pixel = k AT THAT PIXEL, bit for bit.  Single-device contexts only.  No frame kernel is involved.
 *
 * The rule.  State per pixel: the fold's sum[3], one float sq, one uint32 count.  Step for sample s with colour (r, g, b) and n = s + 1,
 * every operation in float32 with one rounding:
 *   sum_c   = (s == 0 ? 0.0f : sum_c) + c
 *   sq      = (s == 0 ? 0.0f : sq) + ((r*r + g*g) + b*b)
 *   inv     = 1.0f / (float)n
 *   mean_c  = sum_c * inv
 *   q       = sq * inv
 *   mm      = (mean_r*mean_r + mean_g*mean_g) + mean_b*mean_b
 *   var     = q - mm
 *   bound   = ((threshold*threshold) * (float)n) * (mm > floor ? mm : floor)
 *   converged = (var <= bound)
 *   count   = n
 *   keep    = (n < max_samples) && !(n >= min_samples && converged)
 * converged is false when either side is NaN, and a negative var converges.  In words: the squared standard error of the mean is at most
 * threshold^2 times max(|mean|^2, floor); no division, no square root.  A pixel with a NaN or infinite sample never converges and runs to
 * max_samples; a pixel of identical samples has var <= 0 and stops at min_samples.
 * crt_adaptive: size must be sizeof(crt_adaptive), min_samples >= 1, max_samples >= min_samples, threshold and floor >= 0 and finite:
 *   anything else is CRT_ERR_INVALID.  crt_adaptive_defaults: 4, 64, 0.05f, 1e-4f.
 * crt_adaptive_step_device: for i < n and pixel p = d_pixels ? d_pixels[i] : i, the step above on d_sum[3p ..], d_sq[p], d_counts[p] with the
 *   colour d_rgb[3i ..] (d_mean[3p ..], where d_mean != NULL, receives the means), and d_next_pixels[0 .. *d_next_n) = the pixels whose keep
 *   is true IN THE ORDER THEY HAD (stable: a list that started as "all pixels" stays ascending; no atomic decides a position, so the list is
 *   the same on every run).  d_sum and d_mean are width * height * 3 floats, d_sq width * height floats, d_counts width * height uint32;
 *   d_next_pixels holds at least n entries and must not alias d_pixels; d_next_n is one uint32 word; d_work is the caller's, at least
 *   crt_adaptive_work_bytes(n) bytes (wave masks, workgroup counts and offsets), aligned to 8 bytes.  The NULL and n rules are
 *   crt_accumulate_samples_device's: with d_pixels == NULL, n must be width * height.  n > 2^32 - 1, a NULL array other than d_pixels and
 *   d_mean, and sample == 2^32 - 1 are CRT_ERR_INVALID.  n == 0 is CRT_OK: it writes *d_next_n = 0 and nothing else.  An index outside the
 *   frame is skipped and not kept; a pixel that is not listed is not touched in any array; THE PIXELS OF ONE CALL MUST BE DISTINCT.  Three
 *   launches on `stream` -- step, a prefix sum over the workgroups' counts by one workgroup, scatter -- and nothing else: no wait, no
 *   allocation, no readback, so the call can be captured into a hipGraph and composes with its two siblings and crt_shoot_rays_gi_enqueue.
 * crt_render_adaptive: crt_render_progressive's loop with a list.  Pass s shoots the active list A_s, A_0 being every pixel: the rays and
 *   keys of sample s of the listed pixels, crt_shoot_rays_gi_device's path in its usual passes, the step into context-owned sum, sq and
 *   counts with the mean into the persistent colour buffer (crt_read_quantized works unchanged); A_(s+1) is the kept pixels.  Its length
 *   is read back through pinned memory, 4 bytes, once per pass.  A pass with an empty list launches nothing; passes at s >= max_samples
 *   are empty by construction.  crt_progressive_samples counts PASSES here and advances by n_passes regardless, so the first_pass rule is
 *   crt_render_progressive's: 0 starts a new frame, otherwise it must equal the count.  `adaptive` is latched at first_pass == 0: a
 *   continuing call whose adaptive differs is CRT_ERR_INVALID.  Continuing an adaptive frame with crt_render_progressive, or a uniform
 *   one with crt_render_adaptive, is CRT_ERR_INVALID, and the message says which kind of frame is under way.  Everything
 *   crt_render_progressive refuses is refused here, with nothing changed; n_passes == 0 is CRT_OK and touches nothing; crt_set_camera and
 *   crt_render* reset it.  out_rgb (height * width * 3 floats) and out_counts (height * width uint32, the samples each pixel holds) are
 *   host memory and may be NULL; the call returns when both are there.  It leaves crt_stats, the ray queues' sizing and fallback_frames
 *   alone; crt_get_shoot_stats describes the last non-empty pass.
 * crt_progressive_active: the pixels the next pass would shoot (every pixel while a uniform frame is under way); 0 when the frame is done
 *   or none is under way. */
typedef struct crt_adaptive {
    uint32_t size;          /* sizeof(crt_adaptive) */
    uint32_t min_samples;   /* >= 1 */
    uint32_t max_samples;   /* >= min_samples */
    float threshold;        /* >= 0, finite */
    float floor;            /* >= 0, finite: |mean|^2 below which the error is absolute */
} crt_adaptive;
void crt_adaptive_defaults(crt_adaptive *a);   /* 4, 64, 0.05f, 1e-4f */
size_t crt_adaptive_work_bytes(uint64_t n);    /* wave masks + workgroup counts + offsets for a list of n entries */
int crt_adaptive_step_device(crt_ctx *ctx, const float *d_rgb, const uint32_t *d_pixels, uint64_t n, uint32_t sample, const crt_adaptive *adaptive,
                             float *d_sum, float *d_sq, float *d_mean, uint32_t *d_counts, uint32_t *d_next_pixels, uint32_t *d_next_n, void *d_work,
                             void *stream);
int crt_render_adaptive(crt_ctx *ctx, const crt_options *options, const crt_adaptive *adaptive, uint32_t first_pass, uint32_t n_passes,
                        float *out_rgb, uint32_t *out_counts);
uint64_t crt_progressive_active(const crt_ctx *ctx);

/* ---- Denoising: a spatial, variance-guided, edge-avoiding a-trous wavelet filter for GI frames of a few samples per pixel -- SVGF's
 * spatial half, with no temporal part.  It uses what the calls above already compute: the per-pixel variance that the adaptive fold's
 * sum[3], sq and count stand for, and the first hit of every pixel (crt_camera_rays_device + crt_trace_rays_device: point, normal, t, mesh)
 * as edge-stopping guides.  Kernels: csrc/kernel_denoise.h; the rule, one header for host and device: csrc/denoise_rule.h.  It is
 * additive: no frame, query, radiance, progressive or adaptive kernel is involved, and a frame that is denoised and then continued is the
 * same frame as before.  Single-device contexts only.
 *
 * The rule.  Every line is one float32 operation with one rounding, in the order written.
 * Definitions.  finite(x) is (x - x) == 0.0f.  A pixel is usable when its three colour channels and its variance are all finite.  A guide is
 *   {n[3], x[3], t, mesh}, taken from a crt_hit: normal, point, t and mesh; mesh = 0xFFFFFFFF when hit == 0.
 *   h = {1/16, 1/4, 3/8, 1/4, 1/16}.  g3 = {1,2,1; 2,4,2; 1,2,1} as floats.
 * From the fold's state (crt_sample_variance_device).  n = count.  When n == 0, colour and variance are 0.  Otherwise:
 *     inv = 1.0f / (float)n
 *     C_c = sum_c * inv                              // the adaptive rule's mean
 *     q   = sq * inv
 *     mm  = (C_r*C_r + C_g*C_g) + C_b*C_b
 *     var = q - mm
 *     V   = (var > 0 ? var : 0) * inv                // the variance OF THE MEAN
 * Iteration k (step = 1 << k), centre p = (y, x).  A centre that is not usable passes through: C' = C, V' = V.  Otherwise:
 *     vnum = 0; vden = 0
 *     for dy in -1..1, dx in -1..1 (row-major), q = (y+dy, x+dx) inside the frame and finite(V_q):
 *         vnum = vnum + g3[dy+1][dx+1] * V_q
 *         vden = vden + g3[dy+1][dx+1]
 *     vp  = vnum / vden
 *     s2  = sigma_colour * sigma_colour
 *     den = s2 * vp + floor
 *     tol = sigma_plane * t_p
 *     acc = {0,0,0}; accv = 0; wsum = 0
 *     for dy in -2..2, dx in -2..2 (row-major), q = (y + dy*step, x + dx*step) in signed arithmetic:
 *         skip q outside the frame
 *         skip q not usable
 *         skip q with mesh_q != mesh_p
 *         if mesh_p is a hit:
 *             d  = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z
 *             d  = d > 0 ? d : 0
 *             d  = d * d, normal_squarings times
 *             e  = (n_p.x*(x_q.x - x_p.x) + n_p.y*(x_q.y - x_p.y)) + n_p.z*(x_q.z - x_p.z)
 *             ae = fabsf(e)
 *             skip unless ae <= tol                  // a NaN skips
 *             wz = tol > 0 ? 1.0f - ae / tol : 1.0f
 *             g  = d * wz
 *         else:
 *             g = 1.0f
 *         dr, dg, db = C_q - C_p
 *         d2 = (dr*dr + dg*dg) + db*db
 *         wl = den / (den + d2)
 *         w  = ((h[dy+2] * h[dx+2]) * g) * wl
 *         acc_c = acc_c + w * C_q,c
 *         accv  = accv + (w*w) * V_q
 *         wsum  = wsum + w
 *     if wsum > 0:
 *         inv = 1.0f / wsum
 *         C'_c = acc_c * inv
 *         V'   = accv * (inv * inv)
 *     else:
 *         pass through
 *   iterations == 0 copies input to output.  A NaN that arises from overflow is whatever these lines give.
 * Known limits.  There is no albedo demodulation, because the library has no albedo query: texture detail inside one mesh is protected by
 *   the colour weight alone -- in THIS call; crt_render_denoised_split ("Split GI frames", below) filters the indirect light only and
 *   adds the direct light, which carries the texels, back untouched.  Reflections in a flat mirror are guided by the mirror's own plane
 *   while crt_guide_bounces(ctx) is 0, the default: "Chain guides", below, gives such pixels the guide of the surface they show.  With count == 1 every variance is 0, so
 *   the filter hardly smooths: use at least 2 samples -- or crt_set_variance_estimate ("Variance estimate", below), which estimates the
 *   variance of such pixels from their neighbours.
 * crt_denoise: size must be sizeof(crt_denoise) = 24, iterations <= 8, normal_squarings <= 16, sigma_colour and sigma_plane >= 0 and finite,
 *   floor > 0 and finite: anything else is CRT_ERR_INVALID, with nothing enqueued.  crt_denoise_defaults: 4, 5, 2.0f, 0.02f, 1e-6f.
 * crt_sample_variance_device: for i < n_pixels the lines "from the fold's state" on d_sum[3i ..], d_sq[i], d_counts[i] -- the arrays
 *   crt_adaptive_step_device keeps -- into d_mean[3i ..] and d_var[i].  n_pixels == 0 is CRT_OK and touches nothing; a NULL array is
 *   CRT_ERR_INVALID.
 * crt_denoise_device: `iterations` iterations of the rule on the width x height image d_rgb (3 floats a pixel), d_var (one float a pixel) with
 *   the guides of d_hits (one crt_hit a pixel, row-major; e.g. what crt_trace_rays_device wrote for crt_camera_rays_device's rays), into
 *   d_out_rgb and d_out_var.  width and height are the CALLER'S, not the scene's: the primitive serves any image with guides.  d_out_var may
 *   be NULL.  d_out_rgb may be d_rgb (and d_out_var d_var), because the pack kernel copies first; any other overlap is not allowed.  d_work
 *   is the caller's, at least crt_denoise_work_bytes(width, height) bytes (64 a pixel: a 32-byte guide record and two 16-byte {r, g, b, V}
 *   records that ping-pong between the iterations), aligned to 16 bytes; nothing may overlap it.  CRT_ERR_INVALID, with nothing enqueued:
 *   an invalid crt_denoise (above), width * height >= 2^31, a NULL required array, a misaligned d_work.  width * height of 0 with non-NULL
 *   arrays is CRT_OK and touches nothing.  One launch to pack and one an iteration (iterations == 0: device-to-device copies).
 * Both device calls only ENQUEUE on `stream` (a hipStream_t, NULL = default): no wait, no allocation, no readback.  They compose with
 *   crt_shoot_rays_gi_enqueue, crt_adaptive_step_device and crt_trace_rays_device on one stream.
 * crt_render_denoised acts on the ADAPTIVE frame under way or finished (crt_progressive_samples(ctx) > 0, started by crt_render_adaptive).
 *   Anything else is CRT_ERR_INVALID, with a message that says why; a uniform crt_render_progressive frame keeps no sq: the message says
 *   to use crt_render_adaptive with min_samples = max_samples.  The guides are the first hits of the camera's centre rays --
 *   crt_camera_rays_device's rays traced as CRT_RAY_PRIMARY through crt_trace_rays_device's path (crt_get_query_stats describes that
 *   trace) --, traced at a frame's first denoise call and kept until the frame is reset (crt_set_camera, crt_render*, a new first pass).
 *   Then variance, pack and the iterations run into a context-owned buffer of their own, and the result goes to out_rgb (height * width * 3
 *   floats) and / or out_rgb8 (crt_quantize_device's rule); host memory, either may be NULL; the call returns when they are there.  It
 *   leaves the persistent colour buffer, sum, sq and counts, the active list, crt_progressive_samples, crt_stats and the ray queues'
 *   sizing exactly as they were, so a frame can be denoised after any pass and continued.  Its buffers are allocated on first use and
 *   freed by crt_destroy. */
typedef struct crt_denoise {
    uint32_t size;              /* sizeof(crt_denoise) = 24 */
    uint32_t iterations;        /* 0..8 */
    uint32_t normal_squarings;  /* 0..16 */
    float sigma_colour;         /* >= 0, finite: colour distances are weighed against sigma_colour^2 x the local variance of the mean */
    float sigma_plane;          /* >= 0, finite: a tap may lie sigma_plane x t off the centre's tangent plane */
    float floor;                /* > 0, finite: added to that variance term, so that a pixel of variance 0 still averages with its equals */
} crt_denoise;
void crt_denoise_defaults(crt_denoise *d);       /* 4, 5, 2.0f, 0.02f, 1e-6f */
size_t crt_denoise_work_bytes(uint32_t width, uint32_t height);
int crt_sample_variance_device(crt_ctx *ctx, const float *d_sum, const float *d_sq, const uint32_t *d_counts, uint64_t n_pixels, float *d_mean,
                               float *d_var, void *stream);
int crt_denoise_device(crt_ctx *ctx, const crt_denoise *denoise, uint32_t width, uint32_t height, const float *d_rgb, const float *d_var,
                       const crt_hit *d_hits, float *d_out_rgb, float *d_out_var, void *d_work, void *stream);
int crt_render_denoised(crt_ctx *ctx, const crt_denoise *denoise, float *out_rgb, uint8_t *out_rgb8);

/* ---- Temporal accumulation: SVGF's temporal half for a camera that moves through a static scene.  A pixel's first hit is projected into
 * the previous frame's camera, the previous frame's accumulated moments are fetched there with a bilinear tap whose four corners are
 * tested against the pixel's own guide (mesh, normal, plane), and what survives is merged with this frame's moments by sample count.  It
 * uses what the calls above compute: the adaptive fold's sum[3], sq and count, and the first hit of every pixel.  Kernel:
 * csrc/kernel_temporal.h; the rule, one header for host and device: csrc/temporal_rule.h.  It is additive: no frame, query, radiance,
 * progressive, adaptive or denoise kernel is involved.  Single-device contexts only.
 *
 * The rule.  Every line is one float32 operation with one rounding, in the order written; there is no exp, pow or sqrt, and floorf is exact.
 * Records.  A history pixel is 64 bytes, aligned 16: {n[3], t, x[3], mesh, c[3], m2, weight, pad[3]}.  n[3], t, x[3], mesh is the guide of
 *   the frame that wrote it (the denoiser's guide; mesh = 0xFFFFFFFF is a miss), c[3] the accumulated mean colour, m2 the
 *   accumulated mean of r*r + g*g + b*b, weight the number of samples the record stands for, as a float; pad is written as 0.  A tap reads it
 *   with four 16-byte loads from one 64-byte half line.  A pose is {position[3], matrix[9]}, what crt_set_camera takes: (o, m) below.
 *   finite(x) is (x - x) == 0.0f.
 * Pixel p = (y, x) of a width x height frame, with the guide G_p = {n_p, t_p, x_p, mesh_p} of the pixel's crt_hit, the fold's state sum[3],
 *   sq, count, the previous pose (o, m) and the previous history array:
 *   current:
 *     n_c = (float)count
 *     count == 0: C_c = 0, q_c = 0
 *     else: inv = 1.0f / n_c; C_c = sum_c * inv; q_c = sq * inv
 *   reproject:
 *     no history array, or mesh_p is a miss: no history (n_h = 0, valid = 0)
 *     w_j = x_p.j - o.j, j = 0..2
 *     v_i = (w_0*m[3i] + w_1*m[3i+1]) + w_2*m[3i+2], i = 0..2
 *     depth = 0.0f - v_2
 *     skip unless depth > 0                          // a NaN skips
 *     sx = v_0 / depth; sy = v_1 / depth
 *     aspect = (float)width / (float)height
 *     sx = sx / aspect
 *     fx = ((sx + 1.0f) * 0.5f) * (float)width - 0.5f
 *     fy = ((1.0f - sy) * 0.5f) * (float)height - 0.5f
 *     skip unless fx > -1.0f && fx < (float)width && fy > -1.0f && fy < (float)height
 *     x0 = floorf(fx); y0 = floorf(fy)
 *     ax = fx - x0; ay = fy - y0
 *     bx = 1.0f - ax; by = 1.0f - ay
 *     tol = sigma_plane * t_p
 *     acc = {0,0,0}; accq = 0; accn = 0; wsum = 0; valid = 0
 *     taps q in the order (y0,x0) (y0,x0+1) (y0+1,x0) (y0+1,x0+1) with b = by*bx, by*ax, ay*bx, ay*ax:
 *         skip q outside the frame                   // integer comparison, before any address is formed
 *         skip unless weight_q > 0 and c_q[0..2], m2_q, weight_q are all finite
 *         skip unless mesh_q == mesh_p
 *         d = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z
 *         skip unless d >= normal_min
 *         e = (n_p.x*(x_q.x - x_p.x) + n_p.y*(x_q.y - x_p.y)) + n_p.z*(x_q.z - x_p.z)
 *         skip unless fabsf(e) <= tol
 *         wsum = wsum + b
 *         acc_c = acc_c + b * c_q,c
 *         accq = accq + b * m2_q
 *         accn = accn + b * weight_q
 *         valid = valid + 1
 *     wsum > 0: inv = 1.0f / wsum; C_h,c = acc_c * inv; q_h = accq * inv; n_h = accn * inv
 *     else: n_h = 0
 *   merge:
 *     n_h = n_h < max_history ? n_h : max_history
 *     n_h == 0: C = C_c, q = q_c, n = n_c            // exactly: a pixel without history is the denoiser's own input
 *     else: n = n_h + n_c; inv = 1.0f / n; a_h = n_h * inv; a_c = n_c * inv
 *           C_c' = a_h * C_h,c + a_c * C_c,c
 *           q = a_h * q_h + a_c * q_c
 *     n == 0: C = 0, q = 0, V = 0
 *     else: mm = (C_r*C_r + C_g*C_g) + C_b*C_b
 *           var = q - mm
 *           V = (var > 0 ? var : 0) * (1.0f / n)
 *   write:
 *     next[p] = {G_p, C, q, n}; out_rgb[p] = C; out_var[p] = V; out_valid[p] = valid (0..4)
 *   The matrix product is the transpose of getRay's row-vector product: the reference's camera matrices are products of rotations, whose
 *   inverse is the transpose.  A non-finite current sample gives a non-finite record; the next frame skips such a record as a tap, so a NaN
 *   lives for one frame.
 * Known limits.  A miss pixel keeps no history.  A matrix that is not a rotation reprojects wrongly.  The geometry tests reject most of
 *   those taps, but not a slide within one plane.  Reflections are reprojected as if painted on the mirror, with or without chain guides (below).  The history holds the
 *   unfiltered moments: the filtered colour is not fed back.  Texture detail is reprojected and filtered with the noise in this call;
 *   crt_render_accumulated_split ("Split GI frames", below) does both to the indirect light only.
 * crt_temporal: size must be sizeof(crt_temporal) = 16, max_history > 0 and finite, normal_min finite, sigma_plane >= 0 and finite:
 *   anything else is CRT_ERR_INVALID, with nothing enqueued.  crt_temporal_defaults: 64.0f, 0.9f, 0.02f.
 * crt_temporal_device: the rule for every pixel of a width x height image of the caller's: d_sum (3 floats a pixel), d_sq and d_counts --
 *   the arrays crt_adaptive_step_device keeps --, d_hits (one crt_hit a pixel, row-major; e.g. what crt_trace_rays_device wrote for
 *   crt_camera_rays_device's rays), the previous frame's records d_prev and its pose prev_pose (host memory, read before the call returns),
 *   into d_next, d_out_rgb (3 floats a pixel), d_out_var (one float) and d_out_valid (one byte).  d_prev may be NULL, which means no
 *   history; prev_pose is then ignored and may be NULL.  d_out_var and d_out_valid may be NULL.  d_next must not be d_prev; no output may
 *   overlap an input or another output.  CRT_ERR_INVALID, with nothing enqueued: an invalid crt_temporal (above), width * height >= 2^31,
 *   a NULL required array, d_prev without prev_pose, d_next == d_prev, d_next or d_prev not aligned to 16 bytes.  width * height of 0
 *   with non-NULL arrays is CRT_OK and touches nothing.  It only ENQUEUES on `stream` (a hipStream_t, NULL = default): one launch, no wait,
 *   no allocation, no readback.  It composes with crt_adaptive_step_device, crt_trace_rays_device and crt_denoise_device on one stream:
 *   frame k's d_next is frame k+1's d_prev.
 * crt_render_accumulated acts on the ADAPTIVE frame under way or finished and refuses exactly what crt_render_denoised refuses, beside an
 *   invalid crt_temporal and, where `denoise` is not NULL, an invalid crt_denoise.  The guides are crt_render_denoised's guides: traced once
 *   a frame and shared between the two calls.  The context owns two history slots, allocated on first use and freed by crt_destroy:
 *   `previous`, the last FRAME's records and that frame's pose, and `current`, what calls on this frame write.  A frame is identified by
 *   a serial number that advances wherever the guides are dropped: crt_set_camera, crt_render*, a new first pass.  When a call finds that
 *   the serial has changed since `current` was written, `current` becomes `previous` first.  So every call on one frame merges the SAME
 *   previous history with the frame's state as it stands: two calls on an unchanged frame give the same bits, and a call after pass 3 and
 *   another after pass 8 do not count the frame twice.  After the merge, denoise != NULL runs crt_denoise_device's launches on the merged
 *   colour and variance (NULL: no spatial filter).  The result goes to out_rgb (height * width * 3 floats), out_rgb8 (crt_quantize_device's
 *   rule) and out_valid (the valid taps per pixel, height * width bytes); host memory, any of the three may be NULL; the call returns when
 *   they are there.  It leaves alone everything crt_render_denoised leaves alone, so a frame can be accumulated after any pass and
 *   continued, and crt_render_denoised's own result is unchanged by it.  The history survives crt_set_camera, which is its purpose;
 *   crt_history_reset drops it (the next frame is a first frame again), and crt_history_frames counts the frames merged since the last
 *   reset.  Giving consecutive frames different gi_seed values is the CALLER'S job: the same seed and camera give the same samples again,
 *   and merging a frame with its own copy adds nothing. */
typedef struct crt_temporal {
    uint32_t size;       /* sizeof(crt_temporal) = 16 */
    float max_history;   /* > 0, finite: a record stands for at most this many samples when it is merged */
    float normal_min;    /* finite: a tap's normal must have at least this cosine with the pixel's */
    float sigma_plane;   /* >= 0, finite: a tap may lie sigma_plane x t off the pixel's tangent plane */
} crt_temporal;
typedef struct crt_history_pixel {
    float n[3], t, x[3];
    uint32_t mesh;
    float c[3], m2, weight, pad[3];
} crt_history_pixel;     /* 64 bytes; arrays of it must be aligned to 16 bytes */
typedef struct crt_camera_pose {
    float position[3];
    float matrix[9];
} crt_camera_pose;
void crt_temporal_defaults(crt_temporal *t);   /* 64.0f, 0.9f, 0.02f */
int crt_temporal_device(crt_ctx *ctx, const crt_temporal *temporal, uint32_t width, uint32_t height, const crt_camera_pose *prev_pose,
                        const crt_history_pixel *d_prev, const float *d_sum, const float *d_sq, const uint32_t *d_counts, const crt_hit *d_hits,
                        crt_history_pixel *d_next, float *d_out_rgb, float *d_out_var, uint8_t *d_out_valid, void *stream);
int crt_render_accumulated(crt_ctx *ctx, const crt_temporal *temporal, const crt_denoise *denoise /* NULL: no spatial filter */, float *out_rgb,
                           uint8_t *out_rgb8, uint8_t *out_valid);
int crt_history_reset(crt_ctx *ctx);
uint32_t crt_history_frames(const crt_ctx *ctx);

/* ---- Split GI frames: denoise and accumulate the INDIRECT light only.  The reference's calculateDiffusion (RayTracer.cpp:300-356) gives a
 * diffuse hit  colour = (sum over lights of k * base + sum of the GI sample rays' colours) * (1 / (GI_SAMPLE_SIZE + 1)):  the texture /
 * albedo `base` multiplies the direct term alone, so dividing a pixel by its albedo would stamp the inverse texture into the indirect
 * light.  The split that fits is ADDITIVE: a sample is cut into its direct part -- deterministic for a given ray; it carries every texel
 * and every hard shadow edge -- and the rest, the only part with Monte-Carlo noise.  The rest is filtered and reprojected, and the direct
 * part is added back untouched.  Kernels: csrc/kernel_split.h (radiance_keep_direct, split_fold, split_recombine); the rule, one header
 * for host and device: csrc/split_rule.h; tests/split_sets.py restates it.  Every line below is one float32 operation
 * (-ffp-contract=off).  Single-device contexts only.
 * crt_shoot_rays_gi_split / crt_shoot_rays_gi_split_device: crt_shoot_rays_gi / crt_shoot_rays_gi_device with one more output, direct
 *   (3 floats a ray); rgb is bit for bit what the unsplit call writes.  direct[i] depends on the level-0 status of ray i (after shootRay's
 *   entry normalisation), read behind level 0's lighting and before the up-sweep, when the level's colour array holds L, a DIFFUSE
 *   record's direct light:
 *     CRT_SHADE_DIFFUSE                       direct_c = L_c * gi_inv, gi_inv = 1.0f / (float)(gi_sample_size + 1)
 *     CRT_SHADE_BACKGROUND                    direct_c = the ray's whole colour (a miss or a constant material: no noise but its jitter's)
 *     CRT_SHADE_RECURSES, CRT_SHADE_INVALID   direct_c = 0: a mirror's or glass's whole colour is "rest"
 *   A call that runs in several passes writes each pass's slice.  A NULL direct with n > 0 is CRT_ERR_INVALID, beside everything the
 *   unsplit call refuses, with nothing enqueued.  The enqueue-only variants (crt_shoot_rays_gi_enqueue) have NO split form.
 * crt_split_fold_device: one step of the split's fold for entry i < n, pixel p = d_pixels ? d_pixels[i] : i:
 *     r_c      = rgb[3i+c] - direct[3i+c]
 *     dsum_c   = (sample == 0 ? 0.0f : dsum_c) + direct[3i+c]
 *     rsum_c   = (sample == 0 ? 0.0f : rsum_c) + r_c
 *     rsq      = (sample == 0 ? 0.0f : rsq) + ((r_r*r_r + r_g*r_g) + r_b*r_b)
 *   on d_dsum and d_rsum (3 floats a PIXEL) and d_rsq (one).  (d_pixels, n) follow crt_accumulate_samples_device's rules: without a list
 *   n must be width * height, the pixels of one call must be distinct, an index outside the frame is skipped before any address is formed
 *   from it.  d_rsum, d_rsq and the frame's counts have the shape of crt_adaptive_step_device's sum, sq and counts, so the rest goes
 *   through crt_sample_variance_device, crt_temporal_device and crt_denoise_device as they are.
 * crt_split_recombine_device: for i < n_pixels
 *     count == 0: out_c = filtered_c
 *     else:       inv = 1.0f / (float)count; out_c = filtered_c + dsum_c * inv
 *   d_out may be d_filtered.  Both device calls only ENQUEUE on `stream`: one launch, no wait, no allocation, no readback; a NULL array
 *   with n > 0 is CRT_ERR_INVALID, n == 0 is CRT_OK and touches nothing.
 * crt_render_adaptive_split is crt_render_adaptive's loop with the split shoot and, behind a pass's step, the fold above on the same list
 *   and sample.  Everything crt_render_adaptive produces is that call's bit for bit -- the colour buffer, sum, sq, counts, the lists,
 *   out_rgb, out_counts, crt_progressive_active --, and the stopping rule still sees the whole colour.  The frame is latched as split at
 *   pass 0: continuing a split frame with crt_render_adaptive, or an unsplit one with this call, is CRT_ERR_INVALID.  The three arrays
 *   of the split's state are the context's, allocated on first use and freed by crt_destroy; crt_read_split_state copies them to host
 *   memory (height * width * 3 floats of dsum and of rsum, height * width of rsq; any may be NULL) while a split frame is under way --
 *   dsum times 1 / count is the frame's direct-light layer.
 * crt_render_denoised_split refuses what crt_render_denoised refuses, and a frame that is not split.  crt_sample_variance_device's lines on
 *   (rsum, rsq, counts), the a-trous filter on that mean and variance with the frame's shared guides, the recombine, then out_rgb and
 *   out_rgb8 as crt_render_denoised's.
 * crt_render_accumulated_split is crt_render_accumulated on (rsum, rsq, counts), with the recombine behind the optional filter.  The
 *   direct part's mean is this frame's own and is not accumulated: it has no noise to average.  The history holds the moments of the
 *   REST, which must never meet crt_render_accumulated's records of whole colours: this call owns a second pair of history slots and
 *   poses, under the same serial rule.  The two calls do not disturb each other's history.  crt_history_reset drops both pairs;
 *   crt_history_frames_split counts this pair's frames, crt_history_frames the other's, as before.
 * All three leave the frame readable, as their unsplit siblings do: a frame can be denoised after any pass and continued.
 * Known limits.  Mirrors and glass are all "rest" and are filtered as before -- under first-hit guides, or under chain guides (below) with
 *   crt_set_guide_bounces.  A sample with an infinite channel gives inf - inf = NaN in
 *   the rest, and such a pixel passes through the filter as NaN pixels do.  The output is filtered + dmean by the rule: with 0 iterations
 *   it is not bit-equal to the unsplit mean. */
int crt_shoot_rays_gi_split(crt_ctx *ctx, const crt_ray *rays, const uint32_t *keys, uint64_t n, uint32_t ray_type,
                            const crt_options *options, float *out_rgb, float *out_direct);
int crt_shoot_rays_gi_split_device(crt_ctx *ctx, const crt_ray *d_rays, const uint32_t *d_keys, uint64_t n, uint32_t ray_type,
                                   const crt_options *options, float *d_rgb, float *d_direct, void *stream);
int crt_split_fold_device(crt_ctx *ctx, const float *d_rgb, const float *d_direct, const uint32_t *d_pixels, uint64_t n, uint32_t sample,
                          float *d_dsum, float *d_rsum, float *d_rsq, void *stream);
int crt_split_recombine_device(crt_ctx *ctx, const float *d_filtered, const float *d_dsum, const uint32_t *d_counts, uint64_t n_pixels,
                               float *d_out, void *stream);
int crt_render_adaptive_split(crt_ctx *ctx, const crt_options *options, const crt_adaptive *adaptive, uint32_t first_pass, uint32_t n_passes,
                              float *out_rgb, uint32_t *out_counts);
int crt_read_split_state(crt_ctx *ctx, float *out_dsum, float *out_rsum, float *out_rsq);
int crt_render_denoised_split(crt_ctx *ctx, const crt_denoise *denoise, float *out_rgb, uint8_t *out_rgb8);
int crt_render_accumulated_split(crt_ctx *ctx, const crt_temporal *temporal, const crt_denoise *denoise /* NULL: no spatial filter */,
                                 float *out_rgb, uint8_t *out_rgb8, uint8_t *out_valid);
uint32_t crt_history_frames_split(const crt_ctx *ctx);

/* ---- Chain guides: filter guides that follow mirrors and glass to the surface they show.  The a-trous filter takes its edge-stopping
 * guides from a crt_hit per pixel.  The first hit of a mirror or glass pixel is the wrong guide: every pixel of a flat mirror has the same
 * mesh, normal and plane, so only the colour weight separates the surfaces the mirror shows.  A chain guide is the record of the first
 * diffuse (or constant) surface the pixel's ray reaches through reflective and refractive meshes.  It is additive: a new way to produce
 * guide records; crt_denoise_device and crt_temporal_device take them as they take any crt_hit array.  Kernel: csrc/kernel_guides.h
 * (guide_step), launched by csrc/crt_guides.hip behind the ray queries' walks; tests/guide_sets.py restates the rule.  Single-device
 * contexts only.  No frame, radiance, denoise or temporal kernel is involved.
 *
 * The rule.  Every float operation is float32 with one rounding.
 * Segments.  A pixel's chain starts with the caller's ray, AS GIVEN (crt_trace_rays*' rule: nothing is normalised), traced as the caller's
 *   ray_type: segment 0.  After segment k with closest hit h_k the hit's material decides:
 *     a REFLECTIVE mesh continues with the ray calculateReflection shoots (RayTracer.cpp:366-367);
 *     a REFRACTIVE mesh continues with the transmission ray calculateRefraction shoots, and under total internal reflection with the
 *       reflection ray instead.
 *   These are the children crt_shoot_rays* shoots -- one device function computes them for both, mirror_glass_children of
 *   csrc/kernel_common.h, from segment k's direction as it was traced, h_k's point and normal, options->reflection_bias and
 *   options->refraction_bias --, normalised once more as the child's shootRay entry normalises them (RayTracer.cpp:420).  Reflection
 *   children are CRT_RAY_REFLECTION rays, transmission children CRT_RAY_REFRACTION rays.  Only CRT_RAY_PRIMARY differs in a walk (Ray.cpp:13), so
 *   one launch traces a level's children of both kinds, as CRT_RAY_REFLECTION -- as the levels of crt_shoot_rays* are traced: the same bits.  For a caller's ray that
 *   normalisation leaves as it is, segment k is therefore the ray shootRay traces at depth k along that branch.
 * Termination.  The chain ends at a miss, at a diffuse or constant material, or when k == max_bounces.
 * Guide record, a crt_hit.  point, normal, u, v, triangle and hit are the terminal hit's.  t is the PATH LENGTH ((t_0 + t_1) + ...) + t_k,
 *   one float32 add per segment in that order, so that the filter's tol = sigma_plane * t scales with the whole path.  mesh is TAGGED: with
 *   0 bounces it is the terminal mesh, otherwise terminal_mesh + n_meshes * (1 + mesh of h_0).  The tag keeps a wall seen in a mirror from
 *   being averaged with the same wall seen directly, or seen in another mirror; equality is all the filter asks of mesh (the tag is below
 *   0xFFFFFFFF, the filter's own mark of a miss).  A miss is all-zero with hit == 0, as crt_trace_rays* writes it, after any number of bounces.
 * Status byte, one per ray.  Bits 0-5: the number of bounces k.  Bit 7: the chain was cut at max_bounces on a reflective or refractive
 *   hit; the record is then that hit's.  max_bounces == 0 gives crt_trace_rays_device's records bit for bit.
 * Known limits.  The Fresnel reflection on glass is guided by what lies BEHIND the glass: one guide a pixel follows one branch.  Temporal
 *   reprojection is unchanged: crt_render_accumulated* reprojects first hits, mirrors as if painted (below).  A curved mirror spreads a
 *   surface's taps thinly: neighbouring pixels end on different meshes or far-apart points, and few taps pass the mesh and plane tests.
 * crt_guide_rays_device: the rule for d_rays[0 .. n) into d_out_hits (one crt_hit a ray), d_out_status (one byte; may be NULL) and
 *   d_out_last_rays (the terminal segment's crt_ray, as it was traced; may be NULL).  d_work is the caller's, at least
 *   crt_guide_work_bytes(n) bytes (512 + 120 a ray: the levels' counts, a level's hit records, two compact lists of ray, pixel, path
 *   length and first mesh), aligned to 16 bytes; nothing may overlap it.  Of `options` reflection_bias and refraction_bias are read;
 *   use_gi may be left set and is ignored.  CRT_ERR_INVALID, with nothing enqueued: max_bounces > 63, a NULL d_rays, options or d_out_hits,
 *   a NULL or misaligned d_work, an unknown ray_type, n > 2^30, a scene with n_meshes * (n_meshes + 1) >= 0xFFFFFFFF.  n == 0 is CRT_OK
 *   and touches nothing.
 *   It only ENQUEUES on `stream` (a hipStream_t, NULL = default): no host wait, no allocation once the context's query scratch has seen a
 *   call of this size, no readback the host waits for.  Each bounce is one trace of the live chains -- crt_trace_rays_device's launches,
 *   sized for n and reading the list's length from a device word, as crt_shoot_rays_enqueue's levels do -- and one guide_step launch
 *   behind it, which finalises a pixel's record or appends the chain's next segment to the next level's compact list (one ballot and one
 *   atomic per wave; the capacity of every level is n, so nothing can overflow).  The order in a list may vary from run to run; no pixel's
 *   result does.  4 (max_bounces + 1) launches; a level that ran dry costs empty launches, nothing else.
 *   Inside a stream capture the call follows crt_shoot_rays_enqueue's rule: it makes no HIP call that synchronises, allocates or records an
 *   event, and returns CRT_ERR_INVALID before it enqueues anything if it would need one (a pending crt_render_async frame, an open call, a
 *   reroute list that would have to grow: make the same call once before the capture).  Outside a capture it is an open call like
 *   crt_trace_rays_device: crt_get_query_stats gives rays = n and hits = the segments with a hit, over all levels.
 * crt_guide_rays: the host variant; copies in, runs, copies out and returns when the results are there.  out_status and out_last_rays may
 *   be NULL.
 * crt_set_guide_bounces / crt_guide_bounces: the frame calls' setting, 0 by default; at 0 every call gives the bits it gave before.  With
 *   a value above 0 the SPATIAL FILTER STAGE of crt_render_denoised, crt_render_accumulated and their _split forms runs under the chain
 *   guides of the camera's centre rays (crt_camera_rays_device's rays as CRT_RAY_PRIMARY, with the biases of the frame's pass 0), traced
 *   once a frame and kept beside the first-hit guides.  THE TEMPORAL STAGE KEEPS THE FIRST-HIT GUIDES: with a still camera "as if painted"
 *   is exact, and a terminal point projected into the last camera would lose that.  Setting another value drops the frame's kept guides
 *   (they are traced again by the next call); it does not drop the history and does not advance the frame's serial.  A value above 63 is
 *   CRT_ERR_INVALID, and so is a scene whose mesh tag does not fit. */
size_t crt_guide_work_bytes(uint64_t n);
int crt_guide_rays(crt_ctx *ctx, const crt_ray *rays, uint64_t n, uint32_t ray_type, const crt_options *options, uint32_t max_bounces,
                   crt_hit *out_hits, uint8_t *out_status /* may be NULL */, crt_ray *out_last_rays /* may be NULL */);
int crt_guide_rays_device(crt_ctx *ctx, const crt_ray *d_rays, uint64_t n, uint32_t ray_type, const crt_options *options, uint32_t max_bounces,
                          crt_hit *d_out_hits, uint8_t *d_out_status /* may be NULL */,
                          crt_ray *d_out_last_rays /* may be NULL: the terminal segment's crt_ray */, void *d_work, void *stream);
int crt_set_guide_bounces(crt_ctx *ctx, uint32_t max_bounces);
uint32_t crt_guide_bounces(const crt_ctx *ctx);

/* ---- Variance estimate: SVGF's variance-estimation stage.  The a-trous filter's colour weight is den / (den + d2) with
 * den = sigma_colour^2 x vp + floor: where a pixel's variance is 0 or unreliable -- one sample and no history: the first frame after
 * crt_history_reset, every disoccluded pixel of a moving camera, every pixel the adaptive rule stopped early -- the weight closes and the
 * noise passes through.  Where the number of samples a pixel's moments stand for is below a threshold, this stage replaces the pixel's
 * variance of the mean by a 7x7 cross-bilateral estimate from the moments of geometrically similar neighbours.  Only the variance is
 * replaced; the colour is never touched.  Kernel: csrc/kernel_variance.h (variance_estimate: a 32x8 tile whose 38x14 halo is staged in LDS
 * once, and tiles without a flagged pixel copy); the rule, one header for host and device: csrc/variance_rule.h; tests/variance_sets.py
 * restates it.  It is additive: no frame, query, radiance, denoise, temporal, split or guide kernel is involved, and with the setting off,
 * the default, every call gives the bits it gave before.  Single-device contexts only.
 *
 * The rule.  Every line is one float32 operation with one rounding, in the order written; there is no exp, pow or sqrt.
 * Definitions.  finite(x) is (x - x) == 0.0f.  A moment record is M = {c[3], m2, weight}, the fields of a crt_history_pixel (the record's
 *   own guide fields are not read).  usable(M): weight > 0 and c[0..2], m2, weight all finite.  A guide is G = {n[3], x[3], t, mesh}, taken
 *   from a crt_hit as the denoiser takes it (mesh = 0xFFFFFFFF when hit == 0).  V_in is the incoming
 *   variance of the mean.  The window radius is 3 and is not a setting.
 * Centre p = (y, x) of a width x height image.  It passes through, V' = V_in, when
 *     !usable(M_p), or mesh_p is a miss, or !(weight_p < min_history)
 * Otherwise the centre is FLAGGED:
 *     tol = sigma_plane * t_p
 *     acc = {0,0,0}; accq = 0; wsum = 0
 *     for dy in -3..3, dx in -3..3 (row-major), q = (y+dy, x+dx); the offsets are compared with the room the centre has before a coordinate is formed:
 *         skip q outside the frame
 *         skip q with !usable(M_q)
 *         skip q with mesh_q != mesh_p
 *         d  = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z
 *         d  = d > 0 ? d : 0
 *         d  = d * d, normal_squarings times
 *         e  = (n_p.x*(x_q.x - x_p.x) + n_p.y*(x_q.y - x_p.y)) + n_p.z*(x_q.z - x_p.z)
 *         ae = fabsf(e)
 *         skip unless ae <= tol                      // a NaN skips
 *         wz = tol > 0 ? 1.0f - ae / tol : 1.0f
 *         w  = d * wz
 *         acc_c = acc_c + w * c_q,c
 *         accq  = accq + w * m2_q
 *         wsum  = wsum + w
 *     if wsum > 0:
 *         inv = 1.0f / wsum
 *         Cb_c = acc_c * inv
 *         qb  = accq * inv
 *         mm  = (Cb_r*Cb_r + Cb_g*Cb_g) + Cb_b*Cb_b
 *         var = qb - mm
 *         iw  = 1.0f / weight_p
 *         V'  = (var > 0 ? var : 0) * iw
 *     else:
 *         V' = V_in                                  // a flagged centre with no surviving tap, or a NaN weight sum
 *   The centre is its own tap (dy = dx = 0).  A NaN that arises from overflow or from a non-finite guide is whatever these lines give: a NaN
 *   w makes wsum NaN, and the centre passes through.  The geometry lines are the denoiser's own.
 * Known limits.  A miss pixel is never estimated.  The estimate is spatial: where the neighbourhood is a texture or a shadow edge inside
 *   one mesh and plane, the detail counts as variance and the filter smooths it more; the split calls hand this rule the moments of the
 *   indirect light only.  The window is 7x7 and dense; it does not widen where few taps survive.
 * crt_variance_estimate: size must be sizeof(crt_variance_estimate) = 16, min_history > 0 and finite, normal_squarings <= 16, sigma_plane
 *   >= 0 and finite: anything else is CRT_ERR_INVALID, with nothing enqueued.  crt_variance_estimate_defaults: 4.0f, 5, 0.02f.
 * crt_variance_estimate_device: the rule for every pixel of a width x height image of the caller's: d_moments (one crt_history_pixel a
 *   pixel, row-major, aligned to 16 bytes; c, m2 and weight are read), d_hits (one crt_hit a pixel: the guides), d_var (one float a
 *   pixel: V_in) into d_out_var.  d_out_var may be d_var, because a pixel reads only its own V_in; no other overlap is allowed.
 *   CRT_ERR_INVALID, with nothing enqueued: an invalid crt_variance_estimate (above), width * height >= 2^31, a NULL array, d_moments not
 *   aligned to 16 bytes.  width * height of 0 with non-NULL arrays is CRT_OK and touches nothing.  It only ENQUEUES on `stream` (a
 *   hipStream_t, NULL = default): one launch, no wait, no allocation, no readback; it can be captured into a graph.  It composes on one
 *   stream between crt_temporal_device -- whose d_next is its d_moments and whose d_out_var is its d_var -- and crt_denoise_device.
 * crt_set_variance_estimate / crt_get_variance_estimate: the frame calls' setting, off by default; NULL turns it off.  An invalid struct is
 *   CRT_ERR_INVALID and leaves the setting as it was.  Changing it drops nothing: not the guides, not the history, not the frame's serial.
 *   crt_get_variance_estimate returns 1 and copies the setting to *out (which may be NULL) when it is on, 0 when it is off.  With it on,
 *   crt_render_denoised, crt_render_accumulated and their _split forms run the estimate between the stage that produces colour and variance
 *   and the a-trous filter, under the guides the filter runs under: chain guides when crt_guide_bounces(ctx) > 0, first hits otherwise.
 *   The accumulated calls take the records the merge just wrote to `current` (split: the moments of the rest); with denoise == NULL they
 *   skip the estimate, since there is no spatial stage to serve.  The denoised calls have no records: they run the temporal launch with no
 *   history (d_prev == NULL) into a context-owned scratch record array, allocated on first use and freed by crt_destroy, in place of
 *   crt_sample_variance_device's launch -- by the temporal rule its colour and variance are that call's, bit for bit, and its records are
 *   {G, C_c, q_c, n_c}.  That touches neither history: no ledger, slot or frame count.  Everything else -- the frame, its sums, counts and
 *   lists, crt_stats, the histories -- is left as it is with the setting off, so a frame can still be processed after any pass and
 *   continued. */
typedef struct crt_variance_estimate {
    uint32_t size;              /* sizeof(crt_variance_estimate) = 16 */
    float min_history;          /* > 0, finite: a pixel whose record stands for fewer samples than this is estimated */
    uint32_t normal_squarings;  /* 0..16 */
    float sigma_plane;          /* >= 0, finite: a tap may lie sigma_plane x t off the centre's tangent plane */
} crt_variance_estimate;
void crt_variance_estimate_defaults(crt_variance_estimate *est);   /* 4.0f, 5, 0.02f */
int crt_variance_estimate_device(crt_ctx *ctx, const crt_variance_estimate *est, uint32_t width, uint32_t height,
                                 const crt_history_pixel *d_moments, const crt_hit *d_hits, const float *d_var, float *d_out_var, void *stream);
int crt_set_variance_estimate(crt_ctx *ctx, const crt_variance_estimate *est /* NULL: off */);
int crt_get_variance_estimate(const crt_ctx *ctx, crt_variance_estimate *out /* may be NULL */);

/* ---- Lightmap baking: a mesh's UV texels lit by the radiance queries -- ambient-occlusion and light baking, lightmap texels with bounce
 * light.  The library says where a texel of a mesh's UV layout (crt_scene_desc::vertex_uvs) lies in the world, which triangle owns it and
 * through which probe ray it is lit; the colours are crt_shoot_rays_device's or, with crt_options::use_gi, crt_shoot_rays_gi_device's, so
 * both modes rest on queries that are pinned to the reference.  Kernels: csrc/kernel_bake.h; the rule, one header for host and device:
 * csrc/bake_rule.h.  It is additive: no frame, walk, query, radiance or GI-frame kernel is involved or changed.  Single-device contexts only.
 *
 * The rule (csrc/bake_rule.h, verbatim; tests/bake_sets.py restates it in numpy and the GPU gives its bits):
 * Texel centres.  Texel (row, col) of a W x H map, row 0 the top, has the centre
 *     q.x = ((float)col + 0.5f) / (float)W
 *     q.y = 1.0f - ((float)row + 0.5f) / (float)H
 *   the convention of BitmapTexture::getColor (Texture.cpp:62-72: x = (int)(uv.x * W), y = (int)((1 - uv.y) * H)): a baked map read back
 *   as a bitmap texture lands on the texel that was baked.
 * Coverage.  a, b, c are the x and y of the three vertex_uvs of a triangle, finite(x) is (x - x) == 0.0f:
 *     A = (b.x - a.x) * (c.y - a.y) - (b.y - a.y) * (c.x - a.x)
 *     the triangle covers nothing unless finite(A) and A != 0
 *     box: umin, umax, vmin, vmax the smallest and largest of the three x and of the three y
 *         f0 = umin * (float)W; f1 = umax * (float)W; g0 = (1.0f - vmax) * (float)H; g1 = (1.0f - vmin) * (float)H
 *         each clamped: f < 0 ? 0 : (f > (float)W ? (float)W : f), with (float)H for g
 *         col0 = max((int)f0 - 1, 0); col1 = min((int)f1 + 1, W - 1); row0 = max((int)g0 - 1, 0); row1 = min((int)g1 + 1, H - 1)
 *     only texels with col0 <= col <= col1 and row0 <= row <= row1 are considered: integer comparison, before any address is formed
 *     e1 = (q.x - a.x) * (c.y - a.y) - (q.y - a.y) * (c.x - a.x)
 *     e2 = (b.x - a.x) * (q.y - a.y) - (b.y - a.y) * (q.x - a.x)
 *     e0 = (b.x - q.x) * (c.y - q.y) - (b.y - q.y) * (c.x - q.x)
 *     covered: A > 0 ? (e0 >= 0 && e1 >= 0 && e2 >= 0) : (e0 <= 0 && e1 <= 0 && e2 <= 0)
 *   The test is inclusive, so both triangles at a shared edge cover the texels on it; a NaN covers nothing.
 * Ownership.  A texel's owner is the covering triangle of the mesh with the LOWEST global triangle index; no covering triangle: EMPTY.
 * Record.  With the owner's crt_triangle (v0, v1, v2, the unit face normal nx, ny, nz):
 *     u = e1 / A; v = e2 / A
 *     w = (1.0f - u) - v
 *     point.k = (v0.k * w + v1.k * u) + v2.k * v, k = 0..2
 *     normal = (nx, ny, nz)
 *   u is the weight of vertex 1 and v the weight of vertex 2, the (u, v) of crt_hit and of Texture::getColor.
 * Probe ray.  origin.k = point.k + normal.k * probe_offset; direction.k = -normal.k; the ray type is CRT_RAY_REFLECTION, so back faces
 *   are not culled.  A texel's colour is DEFINED as what shootRay returns for that ray.
 * Keys in the GI mode.  Sample s of texel p = row * W + col has the key crt_gi_mix(crt_gi_mix(gi_seed, p), s); every sample of a texel
 *   uses the same probe ray.  The fold: sum = (s == 0 ? 0 : sum) + c_s; mean = sum * (1.0f / (float)(s + 1)).
 * Dilation.  A pass reads the statuses and colours as they are at the START of the pass.  A texel with status EMPTY takes the colour of
 *   the first of its neighbours, in the order (row - 1, col) (row + 1, col) (row, col - 1) (row, col + 1) (row - 1, col - 1)
 *   (row - 1, col + 1) (row + 1, col - 1) (row + 1, col + 1), whose status is not EMPTY, and becomes DILATED; every other texel keeps
 *   what it has.  A pass copies and does no arithmetic; neighbours outside the map are skipped by integer comparison.  After max(W, H)
 *   passes nothing can change any more, so no more than that are run.
 *
 * Known limits.
 *   * There is no jitter inside a texel: every sample of a texel goes through its centre.
 *   * Overlapping UV charts resolve to the lowest triangle index.
 *   * A probe can meet another surface lying within probe_offset in front of the texel.
 *   * Mirrors and glass are baked as seen along the normal.
 *   * Multi-device contexts are not supported.
 * crt_bake: mesh < n_meshes; width, height and samples > 0; width * height < 2^31; probe_offset finite and > 0; the scene must have been
 *   created with vertex_uvs: anything else is CRT_ERR_INVALID, with nothing enqueued and nothing changed.  crt_bake_defaults: mesh 0,
 *   256 x 256, 1 sample, dilate 2, check_probes 0, probe_offset 1e-3f.  A mesh's triangles are the ones its tree's leaves list.
 * crt_bake_texel, 48 bytes: {point[3], u, normal[3], v, triangle, mesh, status, pad}.  A COVERED texel holds the record above, triangle the
 *   owner's global index, mesh the bake's mesh; an EMPTY texel holds 0 in every float, triangle = 0xFFFFFFFF, the bake's mesh and status 0;
 *   pad is written as 0.
 * crt_bake_texels_device: the records of every texel of the width x height map to d_texels (row-major, aligned to 16 bytes) and the probe
 *   rays of the COVERED texels to d_rays (by texel; an EMPTY texel's ray is not written); samples, dilate and check_probes are not read.
 *   d_work: crt_bake_work_bytes(width, height) bytes, aligned to 16, the caller's; the call keeps the owner plane in it.  It only
 *   ENQUEUES on `stream`: no wait, no allocation, no readback -- except that the FIRST call for a mesh reads the scene's trees back and
 *   allocates the mesh's triangle list, which is kept for the context's life, and that a pending crt_render_async frame is waited for.
 *   Inside a stream capture it refuses with CRT_ERR_INVALID what would do either, before it enqueues anything.  Two runs give the same
 *   bytes: ownership is a minimum, whatever the order of the triangles' waves.  Calls that bake the same mesh must be ordered by the caller
 *   (the mesh's list of large triangles is the context's).
 * crt_bake_dilate_device: `passes` dilation passes on the caller's map d_rgb (width * height * 3 floats) and d_status (width * height
 *   bytes), in place as the caller sees it: the passes ping-pong between the map and d_work (crt_bake_work_bytes bytes, aligned to 16) and
 *   the result ends in d_rgb and d_status.  Enqueue-only: no wait, no allocation, no readback; it can be captured.  passes == 0 is CRT_OK
 *   and touches nothing.
 * crt_bake_lightmap is the frame-level call, synchronous; out_rgb (width * height * 3 floats), out_rgb8 (width * height * 3 bytes),
 *   out_status (width * height bytes) and out_texels (width * height records) are host memory and every one may be NULL.  It rasterises,
 *   reads back ONE count (the covered texels), compacts the covered texels into a row-major list (no atomic decides a position), shoots
 *   the list's probe rays as CRT_RAY_REFLECTION -- use_gi == 0: through crt_shoot_rays_device, `samples` is ignored and a texel is that
 *   colour as it is; use_gi != 0: through crt_shoot_rays_gi_device `samples` times in order under the keys above, with the fold --,
 *   scatters to the map (EMPTY texels are 0), dilates, and quantises with crt_quantize_device.  It shoots in the queries' usual passes, so
 *   the level arrays are bounded by one pass.  With check_probes it also traces the probe rays with crt_trace_rays_device and counts in
 *   crt_bake_stats::probe_self the texels whose probe's closest hit is the owner triangle; otherwise probe_self is 0.
 *   Like the queries it leaves the persistent colour buffer, crt_stats, the ray queues' sizing, the progressive and adaptive frame and
 *   the history exactly as they were, and it waits for a pending crt_render_async frame.  CRT_ERR_INVALID, with nothing changed: what
 *   crt_bake refuses above, NULL options, and whatever the underlying radiance call refuses (max_depth + 1 > 64, gi_sample_size > 64,
 *   levels that cannot be held).  Its arrays are the context's: they grow and are kept.
 * crt_get_bake_stats: the last crt_bake_lightmap call; raster_ms spans the rasteriser, the records, the count's readback and the
 *   compaction, shoot_ms the radiance calls, the scatter and the probes' trace, total_ms the whole call's device work (HIP events). */
typedef struct crt_bake { uint32_t mesh, width, height, samples, dilate, check_probes; float probe_offset; } crt_bake;   /* 28 bytes */
void crt_bake_defaults(crt_bake *b);                /* mesh 0, 256 x 256, 1 sample, dilate 2, check_probes 0, probe_offset 1e-3f */
typedef struct crt_bake_texel { float point[3], u, normal[3], v; uint32_t triangle, mesh, status, pad; } crt_bake_texel;   /* 48 bytes */
enum { CRT_BAKE_EMPTY = 0, CRT_BAKE_COVERED = 1, CRT_BAKE_DILATED = 2 };
typedef struct crt_bake_stats { uint64_t texels, covered, dilated, probe_self; double raster_ms, shoot_ms, total_ms; } crt_bake_stats;
size_t crt_bake_work_bytes(uint32_t width, uint32_t height);   /* 0 when width * height is 0 or >= 2^31 */
int crt_bake_texels_device(crt_ctx *ctx, const crt_bake *bake, crt_bake_texel *d_texels, crt_ray *d_rays, void *d_work, void *stream);
int crt_bake_dilate_device(crt_ctx *ctx, uint32_t width, uint32_t height, uint32_t passes, float *d_rgb, uint8_t *d_status, void *d_work,
                           void *stream);
int crt_bake_lightmap(crt_ctx *ctx, const crt_bake *bake, const crt_options *options, float *out_rgb, uint8_t *out_rgb8, uint8_t *out_status,
                      crt_bake_texel *out_texels);
int crt_get_bake_stats(crt_ctx *ctx, crt_bake_stats *out);

/* ---- Irradiance probes: a volume of SH9 probes made from the radiance queries, sampled at points -- light for what has no lightmap texel:
 * a moving object, a particle, a vertex of a mesh without UVs, a point in the air.  The library says which rays a probe shoots, projects the
 * colours crt_shoot_rays_device or, with crt_options::use_gi, crt_shoot_rays_gi_device returns for them onto nine spherical-harmonic
 * coefficients per channel, optionally marks the probes that stand inside geometry, and interpolates a volume of such records at arbitrary
 * points with normals.  Kernels: csrc/kernel_probes.h; the rule, one header for host and device: csrc/probe_rule.h.  It is additive: no
 * frame, walk, query, radiance, GI-frame or lightmap kernel is involved or changed.  Single-device contexts only (a crt_multi has none of
 * these calls).
 *
 * The rule (csrc/probe_rule.h, verbatim; tests/probe_sets.py restates it in numpy and the GPU gives its bits):
 * Volume.  crt_probe_volume { float origin[3], spacing[3]; uint32_t nx, ny, nz, rays; uint32_t gi_seed; float backface_limit; }.
 *   Probe p = (iz * ny + iy) * nx + ix stands at position.k = origin.k + (float)i_k * spacing.k (the product is rounded, then the sum).
 *   Valid volumes have nx, ny, nz >= 1, 1 <= rays <= 4096, nx * ny * nz < 2^24, finite origin, spacing finite and > 0, and backface_limit
 *   finite in [0, 1].
 * Directions.  Ray j of R = rays is a spherical Fibonacci point, the same set for every probe:
 *     z = 1.0f - (float)(2j + 1) / (float)R
 *     r = sqrtf(max(0, 1.0f - z * z))                   (m = 1.0f - z * z; m > 0 ? m : 0)
 *     t = (float)j * 0.618034f, then t = t - (float)(int32_t)t
 *     phi = t * 6.2831855f
 *     d = (r * crt_cosf(phi), r * crt_sinf(phi), z)      (phi lies in [0, 2 pi], inside the |y| < 120 range of csrc/glibc_sincosf.h)
 *   The ray is {probe position, d}, shot as CRT_RAY_REFLECTION (back faces are not culled).  Its GI key is
 *   crt_gi_mix(crt_gi_mix(gi_seed, p), j).
 * Basis.  Nine real SH functions of a direction (x, y, z), in the fixed order 1, y, z, x, xy, yz, 3z^2 - 1, xz, x^2 - y^2:
 *     Y0 = 0.282095f
 *     Y1 = 0.488603f * y; Y2 = 0.488603f * z; Y3 = 0.488603f * x
 *     Y4 = 1.092548f * (x * y); Y5 = 1.092548f * (y * z); Y7 = 1.092548f * (x * z)
 *     Y6 = 0.315392f * (3.0f * (z * z) - 1.0f)
 *     Y8 = 0.546274f * (x * x - y * y)
 * Projection.  For probe p, coefficient c, channel ch, with L the colour shootRay returned for ray (p, j) and d_j the direction READ FROM
 *   THE RAY ARRAY as given (so the projection also serves a caller's own uniform direction set):
 *     lane partial: part[l], l = 0..63, is the left fold, starting from 0.0f, over j = l, l + 64, ... in increasing order of
 *         L[p][j][ch] * Y_c(d_j)
 *     tree: for step = 32, 16, 8, 4, 2, 1: part[l] = part[l] + part[l + step] for l < step
 *     coef[c][ch] = part[0] * (12.566371f / (float)R)
 *   That is what a wave of 64 lanes does with cross-lane moves; numpy restates it with a reshape.
 * Validity.  Optional, and off when backface_limit == 1.0f.  The same rays go through crt_trace_rays_device; back counts the hits with
 *   (n.x * d.x + n.y * d.y) + n.z * d.z > 0.0f (n the hit's normal), miss the rays without a hit.  The probe is INVALID when
 *   (float)back > backface_limit * (float)R, otherwise VALID.  The counts are integers (ballot and popcount): no order dependence.
 * Record.  crt_probe is 128 bytes, one cache line: 27 floats coef[c][ch], then uint32 rays, back, miss, state, and one pad word written
 *   as 0.  state: CRT_PROBE_INVALID = 0, CRT_PROBE_VALID = 1; the lookup takes every other value as INVALID.  The projection writes
 *   back = 0, miss = 0, state = VALID; the validity pass writes back, miss and state over them.
 * Lookup.  For a point x with normal n, used as given and not normalised:
 *     if any coordinate of x or n is not finite ((v - v) == 0.0f fails): status 0, colour 0; decided before any conversion to an integer
 *     per axis k: g = (x.k - origin.k) / spacing.k, clamped as a float: g < 0 ? 0 : (g > (float)(n_k - 1) ? (float)(n_k - 1) : g)
 *         i0 = (int32_t)g, lowered to n_k - 2 when n_k > 1 and i0 > n_k - 2; f = g - (float)i0
 *         the two corners i0 and i0 + 1 have the weights 1.0f - f and f; with n_k == 1 only i0 = 0 with weight 1.0f exists
 *     corners run in the order dz, dy, dx (dx fastest), with weight w = (wx * wy) * wz
 *     an INVALID corner and a corner of weight 0 are skipped; every corner index is compared with nx * ny * nz as an integer before an
 *         address is formed
 *     W = the left fold of the used weights, S[c][ch] = the left fold of w * coef[c][ch], both starting from 0.0f
 *     no corner used: status 0, colour 0
 *     e[ch] = the left fold over c = 0..8, starting from 0.0f, of (A_c * Y_c(n)) * S[c][ch], A = 1.0f, 0.6666667f (x3), 0.25f (x5)
 *     q = e[ch] / W; out[ch] = q > 0.0f ? q : 0.0f          (a NaN gives 0)
 *     status = the number of corners used (1 to 8)
 *   A_c is the clamped-cosine convolution divided by pi: the result is the colour a white Lambertian surface would show.
 *
 * Known limits.
 *   * Every probe uses the same direction set: there is no per-probe rotation, and re-baked volumes are not blended over time.
 *   * There is no visibility (Chebyshev) term, so light leaks through thin walls.
 *   * SH9 rings under hard directional light.
 *   * The volume is not fed into the frame kernels: a frame does not read it.
 *   * Single-device contexts only.
 * crt_probe_volume_defaults: origin 0, spacing 1, 1 x 1 x 1 probes, 64 rays, gi_seed 0, backface_limit 1.0f (validity off).  A volume that is
 *   not valid is CRT_ERR_INVALID in every call below, with nothing enqueued and nothing changed.
 * The four primitives only ENQUEUE kernels on `stream` (a hipStream_t, NULL = default): no wait, no allocation, no readback, no memset or
 *   copy node, so they can be captured and a captured chain replays in order.  count == 0 or n == 0 is CRT_OK and touches nothing; a NULL
 *   array with work to do is CRT_ERR_INVALID.  d_rays of crt_probe_rays_device and every d_probes must be aligned to 16 bytes.
 * crt_probe_rays_device: the rays of the probes [first, first + count) of the volume, rays * count of them, probe by probe, to d_rays, and
 *   their GI keys to d_keys, which may be NULL: then nothing is written for keys.  first + count > nx * ny * nz is CRT_ERR_INVALID.
 * crt_probe_project_device: the records of `count` probes of `rays` rays each (1 .. 4096; count < 2^24) from the rays d_rays and their
 *   colours d_rgb (3 floats a ray) to d_probes; the direction is read from d_rays as given.  It writes all 128 bytes of a record: the
 *   coefficients, rays, back = 0, miss = 0, state = CRT_PROBE_VALID, pad = 0.  Two runs give the same bytes.
 * crt_probe_validity_device: back, miss and state of `count` records from the rays and the crt_hit records crt_trace_rays_device wrote for
 *   them; the coefficients and `rays` are left as they are.  backface_limit must be finite in [0, 1].
 * crt_probe_irradiance_device: the lookup at n points (d_points, d_normals: 3 floats each; n < 2^31) in the volume's records d_probes
 *   (nx * ny * nz of them) to d_rgb (3 floats a point) and d_status (a byte a point, the corners used; may be NULL).
 * crt_bake_probes is the frame-level call, synchronous; out_probes (host) and d_probes (device, aligned to 16), nx * ny * nz records each,
 *   may each be NULL.  For chunks of probes whose rays fit one bounded scratch area (2^20 rays; at least one probe) it calls
 *   crt_probe_rays_device, then crt_shoot_rays_device -- or, with options->use_gi, crt_shoot_rays_gi_device under the rule's keys; the
 *   volume's gi_seed makes the keys, options->gi_seed is not read --, then crt_probe_project_device, and when backface_limit != 1.0f
 *   crt_trace_rays_device and crt_probe_validity_device.  It calls those entry points as any caller does and waits once a chunk.  Like the
 *   queries it leaves the persistent colour buffer, crt_stats, the ray queues' sizing, the progressive and adaptive frame, the history and
 *   the lightmap bake's state exactly as they were, and it waits for a pending crt_render_async frame.  CRT_ERR_INVALID, with nothing
 *   enqueued: an invalid volume, NULL options, and whatever the underlying radiance call refuses (max_depth + 1 > 64, gi_sample_size > 64,
 *   levels that cannot be held).  Its arrays are the context's own: they grow and are kept.
 * crt_probe_irradiance: the host variant of the lookup: probes, points, normals, out_rgb and out_status (may be NULL) are host memory; it
 *   copies in, runs crt_probe_irradiance_device, copies out and returns when the result is there.
 * crt_get_probe_stats: the last crt_bake_probes call: probes, the probes whose state is not VALID, rays = probes * rays, and HIP-event
 *   times summed over the chunks: shoot_ms the radiance calls, project_ms the projection with the trace and the validity pass, total_ms
 *   the chunks' whole device work. */
typedef struct crt_probe_volume { float origin[3], spacing[3]; uint32_t nx, ny, nz, rays; uint32_t gi_seed; float backface_limit; } crt_probe_volume;   /* 48 bytes */
void crt_probe_volume_defaults(crt_probe_volume *v);   /* origin 0, spacing 1, 1 x 1 x 1, 64 rays, gi_seed 0, backface_limit 1.0f */
typedef struct crt_probe { float coef[9][3]; uint32_t rays, back, miss, state, pad; } crt_probe;   /* 128 bytes */
enum { CRT_PROBE_INVALID = 0, CRT_PROBE_VALID = 1 };
typedef struct crt_probe_stats { uint64_t probes, invalid, rays; double shoot_ms, project_ms, total_ms; } crt_probe_stats;
int crt_probe_rays_device(crt_ctx *ctx, const crt_probe_volume *volume, uint32_t first, uint32_t count, crt_ray *d_rays, uint32_t *d_keys /* may be NULL */,
                          void *stream);
int crt_probe_project_device(crt_ctx *ctx, const crt_ray *d_rays, const float *d_rgb, uint32_t count, uint32_t rays, crt_probe *d_probes, void *stream);
int crt_probe_validity_device(crt_ctx *ctx, const crt_ray *d_rays, const crt_hit *d_hits, uint32_t count, uint32_t rays, float backface_limit,
                              crt_probe *d_probes, void *stream);
int crt_probe_irradiance_device(crt_ctx *ctx, const crt_probe_volume *volume, const crt_probe *d_probes, const float *d_points, const float *d_normals,
                                uint64_t n, float *d_rgb, uint8_t *d_status, void *stream);
int crt_bake_probes(crt_ctx *ctx, const crt_probe_volume *volume, const crt_options *options, crt_probe *out_probes /* host, may be NULL */,
                    crt_probe *d_probes /* device, may be NULL */);
int crt_probe_irradiance(crt_ctx *ctx, const crt_probe_volume *volume, const crt_probe *probes, const float *points, const float *normals, uint64_t n,
                         float *out_rgb, uint8_t *out_status);
int crt_get_probe_stats(crt_ctx *ctx, crt_probe_stats *out);

/* ---- Probe visibility: a depth record per probe and a Chebyshev-weighted lookup, so that an irradiance probe volume does not leak light
 * through walls.  crt_probe_irradiance* above blends a cell's eight corners by trilinear weight alone; the calls of this section lift that
 * limit: crt_probe_depth_device and crt_bake_probes_visible store, per probe and per direction, the first two moments of the distance the
 * probe's rays saw, and crt_probe_irradiance_visible* weights every corner by a one-sided Chebyshev bound on "this probe sees the point".
 * Kernels: csrc/kernel_probe_depth.h; the rule, one header for host and device: csrc/probe_depth_rule.h.  It is additive: crt_bake_probes
 * and crt_probe_irradiance* give the bytes they gave, and no frame, walk, query, radiance, GI-frame or lightmap kernel is involved or
 * changed.  Single-device contexts only.
 *
 * The rule (csrc/probe_depth_rule.h, verbatim; tests/probe_depth_sets.py restates it in numpy and the GPU gives its bits):
 * Depth record.  crt_probe_depth is 512 bytes: 64 pairs (mean, mean2) of float32, pair k = row * 8 + col the texel (col, row) of an 8 x 8
 *   octahedral map of the sphere.  The side is CRT_PROBE_DEPTH_SIDE = 8: a wave's 64 lanes are a probe's 64 texels, and a tap is one
 *   8-byte load.
 * Texel direction.  e_k is the octahedral decode of the texel's centre:
 *     qx = (((float)col + 0.5f) / 8.0f) * 2.0f - 1.0f, qy likewise from row
 *     z = (1.0f - |qx|) - |qy|
 *     (x, y) = (qx, qy) where z >= 0, otherwise the fold ((1.0f - |qy|) * sgn(qx), (1.0f - |qx|) * sgn(qy)), sgn(v) = v >= 0 ? 1.0f : -1.0f
 *     len = sqrtf((x * x + y * y) + z * z); e_k = (x / len, y / len, z / len)
 * Ray distance.  For ray j of the probe with the hit record h crt_trace_rays_device wrote:
 *     r = (h.hit != 0 && h.t < max_distance) ? h.t : max_distance       (a NaN t gives max_distance)
 *     r = r > 0.0f ? r : 0.0f
 *   A back-face hit counts with its own distance.  d_j is the direction READ FROM THE RAY ARRAY as given.
 * Projection.  For texel k, the left folds over j = 0 .. R - 1 in increasing order, each starting from 0.0f:
 *     c = (d_j.x * e_k.x + d_j.y * e_k.y) + d_j.z * e_k.z; c = c > 0.0f ? c : 0.0f
 *     w = c^16 by four squarings (w = c * c; w = w * w; w = w * w; w = w * w)
 *     W = W + w; S1 = S1 + w * r; S2 = S2 + w * (r * r)
 *   The folds run inside one lane: no cross-lane sum, no dependence on arrival.  Where W > 0.0f: mean = S1 / W, mean2 = S2 / W.  Otherwise
 *   (nothing seen, or a NaN) the pair is (max_distance, max_distance * max_distance): the texel saw nothing and hides nothing.
 * Depth tap.  For a direction u (a unit vector, but any floats are answered):
 *     s = (|u.x| + |u.y|) + |u.z|; px = u.x / s; py = u.y / s
 *     where u.z < 0.0f: (px, py) = ((1.0f - |py|) * sgn(px), (1.0f - |px|) * sgn(py)), both from the unfolded values
 *     per axis: g = (p * 0.5f + 0.5f) * 8.0f - 0.5f, clamped as a float: g = g > -0.5f ? g : -0.5f (a NaN gives -0.5f), then
 *         g = g < 7.5f ? g : 7.5f
 *     i = (int32_t)g, lowered by one when (float)i > g: the floor, in [-1, 7]; f = g - (float)i
 *     the four taps (tx, ty) = (ix + a, iy + b), b = 0, 1 outer, a = 0, 1 inner, have the weights (a ? fx : 1.0f - fx) * (b ? fy : 1.0f - fy)
 *     an index outside [0, 7] wraps the octahedral way: tx < 0: tx = 0, ty = 7 - ty; tx > 7: tx = 7, ty = 7 - ty; then, with the new
 *         values, ty < 0: ty = 0, tx = 7 - tx; ty > 7: ty = 7, tx = 7 - tx
 *     k = ty * 8 + tx; it is compared with 64 as an integer before an address is formed
 *     m1 = the left fold over the four taps, starting from 0.0f, of weight * mean_k; m2 likewise of weight * mean2_k
 * Lookup.  csrc/probe_rule.h's lookup in the finite test, the per-axis clamp, the corner order, the trilinear weight wc = (wx * wy) * wz from
 *   the point x, the skipped corners (wc == 0.0f, or not VALID), crt_probe_resolve and status = the corners used.  A used corner is added
 *   with the weight w = wc * vis instead of wc.  With P the corner's crt_probe_position:
 *     b.k = x.k + n.k * normal_bias; v.k = b.k - P.k
 *     dist = sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z)
 *     if dist > 0.0f fails (the point AT the probe, or a NaN): vis = 1.0f
 *     otherwise u.k = v.k / dist; (m1, m2) = the depth tap of the corner's record at u
 *         var = m2 - m1 * m1; var = |var|; var = var > variance_floor ? var : variance_floor        (a NaN gives variance_floor)
 *         if dist <= m1: ch = 1.0f
 *         else e = dist - m1; ch = var / (var + e * e); ch = (ch * ch) * ch
 *         vis = ch > min_weight ? ch : min_weight                                                    (a NaN gives min_weight)
 *   There is no direction ("wrap") factor, so with every pair (max_distance, max_distance^2) and every corner within max_distance of b the
 *   lookup is csrc/probe_rule.h's bit for bit.
 * Parameters.  crt_probe_visibility { uint32_t size; float max_distance, normal_bias, variance_floor, min_weight; }, 20 bytes.  Valid:
 *   size == 20, max_distance finite and > 0, normal_bias finite and >= 0, variance_floor finite and > 0, min_weight finite in (0, 1].
 *   crt_probe_visibility_defaults fills it from a volume:
 *     diag = sqrtf((sx * sx + sy * sy) + sz * sz) of the spacing; max_distance = 1.5f * diag
 *     normal_bias = 0.02f * the smallest spacing
 *     variance_floor = 1e-6f * (max_distance * max_distance)
 *     min_weight = 0.01f
 *
 * Known limits.
 *   * The map's side is fixed at 8: a wall thinner than a texel's footprint at its distance is blurred with what lies behind it.
 *   * There is no direction factor: a probe behind the surface's tangent plane is not down-weighted for that.
 *   * Back-face hits count with their own distance.
 *   * One max_distance per volume.
 *   * Static scenes: nothing blends a re-baked depth record over time.
 *   * Single-device contexts only.
 * crt_probe_visibility_defaults: the parameters above from the volume's spacing; CRT_ERR_INVALID for a NULL or an invalid volume.  A
 *   visibility that is not valid is CRT_ERR_INVALID in every call below, with nothing enqueued and nothing changed.
 * crt_probe_depth_device and crt_probe_irradiance_visible_device only ENQUEUE one kernel on `stream`, as the four primitives above: no wait,
 *   no allocation, no memset or copy node, so they can be captured.  count == 0 or n == 0 is CRT_OK and touches nothing; a NULL array with
 *   work to do is CRT_ERR_INVALID.  Every d_depth must be aligned to 16 bytes.
 * crt_probe_depth_device: the depth records of `count` probes of `rays` rays each (the ranges of crt_probe_project_device) from the rays
 *   d_rays and the crt_hit records d_hits crt_trace_rays_device wrote for them to d_depth; max_distance must be finite and > 0.  It writes
 *   all 512 bytes of a record.  Two runs give the same bytes.
 * crt_probe_irradiance_visible_device: the lookup at n points (n < 2^31) in the volume's records d_probes and depth records d_depth
 *   (nx * ny * nz each) to d_rgb and d_status (may be NULL), as crt_probe_irradiance_device.  crt_probe_irradiance_visible is its host
 *   variant: every array is host memory; it copies in, runs, copies out and returns when the result is there.
 * crt_bake_probes_visible is crt_bake_probes with the depth pass: the same chunk loop, and in every chunk ONE crt_trace_rays_device call
 *   whose hits serve crt_probe_validity_device (when backface_limit != 1.0f) and crt_probe_depth_device (visibility->max_distance).  The SH
 *   records are crt_bake_probes' bytes.  out_depth (host) and d_depth (device, aligned to 16), nx * ny * nz records each, may each be NULL,
 *   as out_probes and d_probes.  It waits as crt_bake_probes waits, leaves what crt_bake_probes leaves as it was, and refuses what it
 *   refuses, and a NULL or invalid visibility.  crt_get_probe_stats then describes this call: project_ms includes the trace and the depth
 *   pass.  crt_debug_set_probe_chunk applies to it. */
typedef struct crt_probe_depth { float moments[64][2]; } crt_probe_depth;   /* 512 bytes: (mean, mean2) of texel row * 8 + col */
typedef struct crt_probe_visibility { uint32_t size; float max_distance, normal_bias, variance_floor, min_weight; } crt_probe_visibility;   /* 20 bytes */
int crt_probe_visibility_defaults(const crt_probe_volume *volume, crt_probe_visibility *visibility);
int crt_probe_depth_device(crt_ctx *ctx, const crt_ray *d_rays, const crt_hit *d_hits, uint32_t count, uint32_t rays, float max_distance,
                           crt_probe_depth *d_depth, void *stream);
int crt_probe_irradiance_visible_device(crt_ctx *ctx, const crt_probe_volume *volume, const crt_probe_visibility *visibility, const crt_probe *d_probes,
                                        const crt_probe_depth *d_depth, const float *d_points, const float *d_normals, uint64_t n, float *d_rgb,
                                        uint8_t *d_status /* may be NULL */, void *stream);
int crt_probe_irradiance_visible(crt_ctx *ctx, const crt_probe_volume *volume, const crt_probe_visibility *visibility, const crt_probe *probes,
                                 const crt_probe_depth *depth, const float *points, const float *normals, uint64_t n, float *out_rgb,
                                 uint8_t *out_status /* may be NULL */);
int crt_bake_probes_visible(crt_ctx *ctx, const crt_probe_volume *volume, const crt_probe_visibility *visibility, const crt_options *options,
                            crt_probe *out_probes /* host, may be NULL */, crt_probe *d_probes /* device, may be NULL */,
                            crt_probe_depth *out_depth /* host, may be NULL */, crt_probe_depth *d_depth /* device, may be NULL */);

/* ---- Probe-lit radiance: the radiance queries' picture with bounce light from an irradiance probe volume.  The three sections above make a
 * light cache; the calls of this section are what reads it: a DIFFUSE record of a radiance query takes, in place of the GI build's
 * gi_sample_size random sample rays, the EXPECTATION of their colours from the volume's SH9 records -- no sample ray is shot, so the result
 * is free of noise and costs about what crt_shoot_rays_device costs.  Mirrors and glass recurse as they do in crt_shoot_rays_gi*, and the
 * diffuse surfaces seen in them are lit from the volume too.  Kernel: csrc/kernel_probe_light.h; the rule, one header for host and device:
 * csrc/probe_lit_rule.h.  It is additive: no existing call changes a byte, no existing kernel gets a new argument, and the frame kernels of
 * crt_render* are not involved.  Single-device contexts only.
 *
 * The rule (csrc/probe_lit_rule.h, verbatim; tests/probe_lit_sets.py restates it in numpy and the GPU gives its bits):
 * Derivation.  In the GI build a DIFFUSE record's colour is (direct + c_0 + ... + c_{S-1}) * (1 / (float)(S + 1)), S = gi_sample_size,
 *   c_i the colour shootRay returns for sample ray i (radiance_combine<true>, csrc/kernel_radiance.h).  gi_sample_direction
 *   (csrc/kernel_lane.h) draws angle1 = pi * u1 and angle2 = 2 pi * u2, forms (cos angle1, sin angle1, 0) in the (right, normal, forward)
 *   frame and rotates it about the normal by angle2: the angle alpha between the sample and the normal is |pi/2 - angle1|, uniform on
 *   [0, pi/2], and the azimuth is uniform.  The density per solid angle is p(omega) = 1 / (pi^2 sin alpha) on the normal's hemisphere; it
 *   depends on the normal alone.  The expectation of one sample's colour, Lbar(x, n) = the integral of L(x, omega) p(omega) d omega, is a
 *   zonal convolution of the incoming radiance, and by Funk-Hecke its SH band factors are
 *       lambda_l = (2 / pi) * the integral over [0, pi/2] of P_l(cos alpha) d alpha:   lambda_0 = 1, lambda_1 = 2 / pi, lambda_2 = 1 / 4
 *   where csrc/probe_rule.h's clamped-cosine lookup has A = 1, 2/3, 1/4.
 * Zonal resolve.  csrc/probe_rule.h's lookup -- or, with a visibility, csrc/probe_depth_rule.h's -- in the finite test, the per-axis clamp,
 *   the corner order, the skipped corners, the weights and the folds W and S[c][ch] (crt_probe_axis, crt_probe_sum_add, the depth tap and
 *   the Chebyshev weight, all unchanged), resolved with the zonal table in place of A:
 *     no corner used: status 0, Lbar = 0
 *     e[ch] = the left fold over c = 0..8, starting from 0.0f, of (Z_c * Y_c(n)) * S[c][ch], Z = 1.0f, 0.63661975f (x3), 0.25f (x5)
 *     q = e[ch] / W; Lbar[ch] = q > 0.0f ? q : 0.0f          (a NaN gives 0)
 *     status = the number of corners used (1 to 8)
 *   x is the record's point and n its normal as the crt_hit holds them (the normal radiance_scatter<true> hands to gi_sample_direction),
 *   used as given and not normalised.  A point or normal that is not finite: status 0, Lbar = 0.
 * Combine.  For a record whose status byte is CRT_SHADE_DIFFUSE, with direct[ch] the colour crt_shade_hits_device left:
 *     ind = (float)S * Lbar[ch]
 *     inv = 1.0f / (float)(S + 1u)
 *     colour[ch] = (direct[ch] + ind) * inv
 *   Every other record keeps its colour's bytes.  A DIFFUSE record of status 0 counts as UNLIT, every other DIFFUSE record as LIT.  With
 *   S = 0 and a finite Lbar the colour is (direct + 0.0f) * 1.0f: direct as a float value.  The indirect term is multiplied by no albedo and
 *   no texture: the reference's is not either (README, "Split GI frames").
 *
 * Known limits.
 *   * The light is the volume's: as smooth as SH9 and the probe spacing make it, with the leaks the lookup in use has, and as old as the
 *     last bake.  Re-baked volumes are not blended over time.
 *   * Lbar is the mean of the GI build's estimator when the volume holds the radiance the sample rays would return; a volume baked with
 *     max_depth - 1 and gi_sample_size S approximates that.  Nothing checks which options a volume was baked with.
 *   * The indirect term carries no albedo (the reference has none).
 *   * The frame kernels of crt_launch.hip do not read the volume: crt_render* give the bytes they gave.
 *   * The query waits once a level: there is no enqueue-only or graph-capturable form.
 *   * Single-device contexts only.
 * crt_probe_light_hits_device only ENQUEUES one kernel on `stream`, as the probe primitives above: no wait, no allocation, no memset or copy
 *   node, so it can be captured.  For each of the n records (n < 2^31) whose d_status byte is CRT_SHADE_DIFFUSE it reads the point and the
 *   normal of d_hits[i] and the direct light d_rgb[3i ..] as crt_shade_hits_device left it, and writes the combined colour over it; every
 *   other record's colour keeps its bytes.  visibility NULL: the plain lookup, and d_depth is not read; otherwise the Chebyshev-weighted
 *   one, and d_depth must not be NULL.  d_counts (may be NULL; two 64-bit words aligned to 8 bytes, which the CALLER clears): [0] += the LIT
 *   records, [1] += the UNLIT ones.  It refuses what crt_probe_irradiance_visible_device refuses -- a NULL or invalid volume, an invalid
 *   visibility, n >= 2^31, a NULL array with work to do, d_probes or d_depth not aligned to 16 bytes --, and gi_sample_size > 64.  n == 0 is
 *   CRT_OK and touches nothing.  Two runs give the same bytes.
 * crt_shoot_rays_lit_device: the colours of n rays on `stream`, as crt_shoot_rays_gi_device takes rays and gives colours (level by level,
 *   GI occlusion rule, one wait a level), run with gi_sample_size = 0 and with the launch above behind every level's lighting launches,
 *   which gets options->gi_sample_size as S.  options->use_gi must be 1.  There are no keys: nothing random is drawn.  With
 *   gi_sample_size = 0 the colours are crt_shoot_rays_gi_device's with gi_sample_size = 0 as float values.  It is CRT_ERR_INVALID, with
 *   nothing enqueued, for what crt_shoot_rays_gi_device refuses, for what the primitive refuses of the volume, and on a stream that is being
 *   captured.  crt_get_shoot_stats describes the call as it describes a crt_shoot_rays_gi_device call.  crt_shoot_rays_lit is its host
 *   variant: rays, probes, depth and out_rgb are host memory (n < 2^31); it copies in, runs on the context's stream, copies out and waits.
 * crt_render_probe_lit: the frame.  The camera's rays (crt_camera_rays_device) of EVERY pixel, shot as CRT_RAY_PRIMARY rays through
 *   crt_shoot_rays_lit_device into the persistent colour buffer, then the quantiser (crt_quantize_device); out_rgb (host, H x W x 3 floats)
 *   and out_rgb8 (host, H x W x 3 bytes) may each be NULL.  d_probes and d_depth are device memory.  It waits for a pending frame, ends a
 *   progressive frame under way as crt_render* do, and returns when the copies have landed.  crt_render_probe_lit_host is the same call for records in HOST memory (probes, depth): it copies them to the
 *   device first.
 * crt_get_probe_lit_stats: the LIT and UNLIT records of the last crt_shoot_rays_lit* or crt_render_probe_lit call, over all its levels and
 *   passes (waits for it); lit + unlit = that call's crt_shoot_stats::shadow_records.  crt_shoot_stats gains nothing. */
typedef struct crt_probe_lit_stats { uint64_t lit, unlit; } crt_probe_lit_stats;
int crt_probe_light_hits_device(crt_ctx *ctx, const crt_probe_volume *volume, const crt_probe_visibility *visibility /* may be NULL */,
                                const crt_probe *d_probes, const crt_probe_depth *d_depth /* may be NULL without a visibility */, const crt_hit *d_hits,
                                const uint8_t *d_status, uint64_t n, uint32_t gi_sample_size, float *d_rgb /* in: direct light, out: the lit colour */,
                                uint64_t *d_counts /* may be NULL */, void *stream);
int crt_shoot_rays_lit_device(crt_ctx *ctx, const crt_ray *d_rays, uint64_t n, uint32_t ray_type, const crt_options *options,
                              const crt_probe_volume *volume, const crt_probe_visibility *visibility /* may be NULL */, const crt_probe *d_probes,
                              const crt_probe_depth *d_depth /* may be NULL without a visibility */, float *d_rgb, void *stream);
int crt_shoot_rays_lit(crt_ctx *ctx, const crt_ray *rays, uint64_t n, uint32_t ray_type, const crt_options *options, const crt_probe_volume *volume,
                       const crt_probe_visibility *visibility /* may be NULL */, const crt_probe *probes, const crt_probe_depth *depth, float *out_rgb);
int crt_render_probe_lit(crt_ctx *ctx, const crt_probe_volume *volume, const crt_probe_visibility *visibility /* may be NULL */, const crt_probe *d_probes,
                         const crt_probe_depth *d_depth /* may be NULL without a visibility */, const crt_options *options, float *out_rgb /* may be NULL */,
                         uint8_t *out_rgb8 /* may be NULL */);
int crt_render_probe_lit_host(crt_ctx *ctx, const crt_probe_volume *volume, const crt_probe_visibility *visibility /* may be NULL */, const crt_probe *probes,
                              const crt_probe_depth *depth /* may be NULL without a visibility */, const crt_options *options, float *out_rgb /* may be NULL */,
                              uint8_t *out_rgb8 /* may be NULL */);
int crt_get_probe_lit_stats(crt_ctx *ctx, crt_probe_lit_stats *out);

/* ---- one scene on several devices of one node, behind the same call (SURVEY.md section 8b "multi-GPU handled inside the
 * context"; the reference's counterpart is the bucket thread pool, RayTracer.cpp:141-158).  One context, host thread and
 * stream per listed device (a device may be listed more than once); the covered 8x8 tiles are dealt round-robin, every
 * device copies its packed tiles to devices[0] over xGMI (peer copy, no collective) and devices[0] scatters them into its
 * persistent colour buffer.  crt_multi_render has crt_render's contract: same pixels, bit for bit. */
typedef struct crt_multi crt_multi;
int crt_multi_create(const crt_scene_desc *scene, const int *devices, uint32_t n_devices, const crt_tuning *tuning, crt_multi **out);
int crt_multi_set_camera(crt_multi *multi, const float position[3], const float matrix[9]);
int crt_multi_render(crt_multi *multi, const crt_options *options, const crt_rect *rects, uint32_t n_rects, float *out_rgb);
int crt_multi_read_quantized(crt_multi *multi, uint8_t *out_rgb8);
/* counters summed over the devices, kernel_ms = the slowest device's, total_ms = wall time of the call */
int crt_multi_get_stats(crt_multi *multi, crt_stats *out);
uint32_t crt_multi_device_count(const crt_multi *multi);
crt_ctx *crt_multi_context(crt_multi *multi, uint32_t part); /* part 0 holds the frame */
const char *crt_multi_last_error(const crt_multi *multi);
/* Parts whose device cannot store into device[0]'s memory (hipDeviceCanAccessPeer / hipDeviceEnablePeerAccess said so at
 * crt_multi_create) copy their tiles through pinned host memory instead of over xGMI: how many there are, and what the
 * runtime answered for each (one line per part, empty when every part has peer access).  Same pixels either way. */
uint32_t crt_multi_staged_parts(const crt_multi *multi);
const char *crt_multi_peer_note(const crt_multi *multi);
int crt_debug_multi_force_staged(crt_multi *multi, int on); /* tests: stage every part, as if no device had peer access */
int crt_debug_multi_fail_next_alloc(crt_multi *multi);       /* tests: the next re-partition stops at a part's buffer with CRT_ERR_NOMEM */
void crt_multi_destroy(crt_multi *multi);

/* ---- the reference's tree built on the GPU (KDTree<T>::build, KDTree.cpp:10-46 / :89-125; BoundingBox.h:60-83): level by
 * level, one thread per (node, element) entry, the same float operations as the reference's split and overlap test, so the
 * result is the reference's tree node for node: same creation-order numbering, same boxes, same leaf lists.
 * element_boxes: 6 floats per element (min xyz, max xyz); root_box likewise.  The built tree is read back through the
 * accessors: boxes 6 floats per node, links 4 words per node (children[0], children[1], parent, number of leaf indexes; none
 * = 0xFFFFFFFF), indexes = the leaves' lists concatenated in node order (the layout of crt_host_tree_dump, crt_host.h). */
typedef struct crt_built_tree crt_built_tree;
int crt_build_tree_device(int device, const float *element_boxes, uint32_t n_elements, const float root_box[6],
                          uint32_t max_depth, uint32_t max_leaf, crt_built_tree **out);
uint32_t crt_built_tree_node_count(const crt_built_tree *tree);
uint64_t crt_built_tree_index_total(const crt_built_tree *tree);
const float *crt_built_tree_boxes(const crt_built_tree *tree);
const uint32_t *crt_built_tree_links(const crt_built_tree *tree);
const uint32_t *crt_built_tree_indexes(const crt_built_tree *tree);
void crt_built_tree_free(crt_built_tree *tree);
const char *crt_build_last_error(void);

/* After a render with collect_counters == 2 on the default (ray-stream) path: out = {box tests, triangle tests} the
 * production kernels executed in the whole render, then the same two for shadow pass 0 alone (the largest kernel).  Fewer than crt_stats' box_tests / tri_tests, which are the reference's: the kernels leave
 * out work that cannot change the result (shadow early exit, one walk per mesh and ray). */
int crt_get_executed_counters(crt_ctx *ctx, uint64_t out[4]);
/* ... and the box tests of the plan loops (csrc/kernel_plan.h: a ray against the top-level leaves, whose boxes sit in scalar
 * registers loaded once per wave -- executed per ray, but with no per-ray fetch): {whole render, of which shadow pass 0}.
 * They are NOT part of the counts above. */
int crt_get_executed_plan_tests(crt_ctx *ctx, uint64_t out[2]);

/* ---- Test hooks: exported by libcrt_hip_test.so only (the product's objects + csrc/crt_testhooks.hip; libcrt_hip.so has none of them):
 * crt_test_pow5, crt_test_gi, crt_bvh_selftest, crt_bvh_census, crt_debug_set_filter_stack, crt_debug_set_query_chunks,
 * crt_debug_multi_force_staged, crt_debug_multi_fail_next_alloc, crt_debug_set_probe_chunk. ---- */
/* Test hook: out[i] = the device build of the restated glibc powf(x[i], 5) (the Fresnel term, RayTracer.cpp:407). */
int crt_test_pow5(int device, const float *x, float *out, uint64_t n);
/* Test hook for the GI mode's arithmetic (csrc/glibc_sincosf.h, csrc/gi_random.h), evaluated on `device`, or by the host
 * build of the same headers when device < 0.  what = 0: out[i] = bits of sinf(a[i] as float); 1: cosf; 2: bits of the
 * uniform number u(key a[i], draw b[i]); 3: mix(a[i], b[i]).  b may be NULL for 0 and 1. */
int crt_test_gi(int device, uint32_t what, const uint32_t *a, const uint32_t *b, uint32_t *out, uint64_t n);

/* Test hook, HOST ONLY (no device is touched): builds the candidate filter of `scene` (csrc/crt_bvh.h) and checks its two promises
 * against brute force for n_rays rays (6 floats each: origin, direction): out = {rays, triangles the reference's test accepts with a
 * finite distance, of which the conservative walk does not reach (must be 0), triangles it accepts with an infinite or NaN distance in
 * a leaf the ray's line passes, of which the miss check does not reach (must be 0), nodes visited by the two walks, structural
 * errors (must be 0)}.  CRT_ERR_INVALID when the scene has no filter. */
int crt_bvh_selftest(const crt_scene_desc *scene, const float *rays, uint32_t n_rays, int primary, uint64_t out[8]);
/* Test hook, HOST ONLY: the shape of that filter: out = {nodes, entries, depth of the binary build, inner nodes on the longest path of
 * the 4-wide hierarchy (a walk's stack is sized 3 x this + 1), triangles verified by the pruned tree walk (BVH_TRI_WALK), 0, 0, 0}.
 * CRT_ERR_INVALID when the scene has no filter. */
int crt_bvh_census(const crt_scene_desc *scene, uint64_t out[8]);
/* Test hook: the filter walks of a live context may use `entries` stack entries from now on -- clamped to [1, what crt_create sized
 * the stacks for], so a large value restores the built size.  Waits for the context's work; changes no pixel (a walk that runs out of
 * stack sends its frame to the queue-less kernel -- crt_stats::fallback_frames -- and its query ray to the reference-order walk). */
int crt_debug_set_filter_stack(crt_ctx *ctx, uint32_t entries);
/* Test hook: the chunk sizes of the queries of a live context from now on, so that a few thousand rays run their chunk loops: rays per
 * round trip of the host variants (2^22), per launch (2^27), per pass of a radiance query (2^22).  0 restores the default; any other
 * value is clamped to [64, the default].  Waits for the context's work; changes no answer and no statistic but kernel_ms. */
int crt_debug_set_query_chunks(crt_ctx *ctx, uint64_t host_rays, uint64_t launch_rays, uint64_t pass_rays);
/* Test hook: crt_bake_probes of a live context takes `probes` probes per chunk from now on, so that a few probes run its chunk loop; 0
 * restores the default (as many as fit its scratch).  Changes no record. */
int crt_debug_set_probe_chunk(crt_ctx *ctx, uint32_t probes);

/* Diagnostics for the development tools under tools/ (no counterpart in the reference; not needed to render):
 * the ray-stream pass's queue counters of the last frame (rays per recursion level, walks handed to the
 * wave-per-ray kernels, ...: the SC_* layout of csrc/kernel_stream.h, at most 512 words). */
int crt_debug_stream_counts(crt_ctx *ctx, uint32_t *out_words, uint32_t max_words);
/* which kernels a production frame of this context runs, e.g. "level0=stream_trace_shade_plan<true>;shadow0=stream_trace_shadow_plan<0u>;
 * levels=heavy_trace_closest<5>" (names as rocprofv3 prints them) */
int crt_describe_kernels(const crt_ctx *ctx, char *out, size_t size);

#ifdef __cplusplus
}
#endif
#endif
