// crt_bake.hip -- lightmap baking (include/crt_hip.h: "Lightmap baking"): crt_bake_defaults, crt_bake_work_bytes, the two enqueue-only
// primitives crt_bake_texels_device and crt_bake_dilate_device, the frame-level crt_bake_lightmap and crt_get_bake_stats.  Kernels:
// csrc/kernel_bake.h; the rule: csrc/bake_rule.h.  The colours are the radiance queries' (crt_shoot_rays_device, crt_shoot_rays_gi_device),
// called as any caller calls them; nothing of a frame, a walk or a query is touched.
#include <memory>

#include "crt_internal.h"
#include "device_array.h"

namespace {
#include "kernel_bake.h"
}  // namespace

static_assert(sizeof(crt_bake) == 28, "include/crt_hip.h says 28");
static_assert(sizeof(crt_bake_texel) == 48 && offsetof(crt_bake_texel, normal) == 16 && offsetof(crt_bake_texel, triangle) == 32 &&
                  offsetof(crt_bake_texel, status) == 40,
              "a record is three 16-byte stores");
static_assert(CRT_BAKE_EMPTY == CRT_BAKE_STATUS_EMPTY && CRT_BAKE_COVERED == CRT_BAKE_STATUS_COVERED && CRT_BAKE_DILATED == CRT_BAKE_STATUS_DILATED,
              "the rule's statuses are the header's");
static_assert(sizeof(crt_node) == 32 && sizeof(crt_triangle) == 64, "the scene's records as crt_create uploads them");

// a mesh's triangles as the reference's tree lists them (ascending, each once), and the rasteriser's large list: made by the first call
// for the mesh, kept for the context's life
struct BakeMesh {
    DeviceArray<uint32_t> tris, large;
    uint32_t n = 0;
};

struct crt_bake_state {
    // host copies of the trees, read back once: which triangles a mesh's leaves list
    std::vector<crt_node> nodes;
    std::vector<uint32_t> leaf_tris;
    std::vector<crt_mesh> mesh_recs;
    bool trees = false;
    std::vector<std::unique_ptr<BakeMesh>> meshes;
    // crt_bake_lightmap: the records, rays and statuses by texel, the primitives' work area, the covered texels' list with its rays, keys and
    // colours, the map and its sum, the quantised map, the probes' hits, the compaction's work and the counts
    DeviceArray<float4> texels, work;
    DeviceArray<crt_ray> rays, list_rays;
    DeviceArray<uint8_t> status, q8;
    DeviceArray<uint32_t> list, keys, counts;
    DeviceArray<float> rgb, map, sum;
    DeviceArray<crt_hit> hits;
    DeviceArray<unsigned long long> list_work;
    uint32_t *pin = nullptr;   // COUNT_WORDS words
    hipEvent_t ev[4] = {};
    crt_bake_stats stats{};
    ~crt_bake_state() {
        if (pin) (void)hipHostFree(pin);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};
enum : uint32_t { COUNT_COVERED = 0, COUNT_DILATED = 1, COUNT_SELF = 2, COUNT_WORDS = 4 };

void bake_destroy(crt_ctx *ctx) {
    delete ctx->bake;
    ctx->bake = nullptr;
}

static int bake_state(crt_ctx *ctx) {
    if (!ctx->bake) ctx->bake = new (std::nothrow) crt_bake_state;
    if (!ctx->bake) { ctx->error = "out of memory"; return CRT_ERR_NOMEM; }
    return CRT_OK;
}

extern "C" void crt_bake_defaults(crt_bake *b) {
    if (!b) return;
    b->mesh = 0;
    b->width = 256; b->height = 256;
    b->samples = 1;
    b->dilate = 2;
    b->check_probes = 0;
    b->probe_offset = 1e-3f;
}

// ---- the work area of the two primitives: crt_bake_texels_device keeps the owner plane in it, crt_bake_dilate_device the second map of
// its ping-pong (colours, then statuses)
static uint64_t align16(const uint64_t bytes) { return (bytes + 15u) & ~15ull; }
extern "C" size_t crt_bake_work_bytes(uint32_t width, uint32_t height) {
    const uint64_t n = (uint64_t)width * height;
    if (n == 0 || n >= CRT_MAX_PIXELS) return 0;
    return (size_t)std::max(align16(4 * n), align16(12 * n) + align16(n));
}

static int bake_check(crt_ctx *ctx, const char *what, const crt_bake *b) {
    if (!b) return refuse(ctx, what, "bake is NULL");
    if (b->mesh >= ctx->scene.n_meshes) return refuse(ctx, what, "mesh " + std::to_string(b->mesh) + " >= n_meshes = " + std::to_string(ctx->scene.n_meshes));
    if (!ctx->scene.vuvs) return refuse(ctx, what, "the scene was created without vertex_uvs");
    if (b->width == 0 || b->height == 0 || b->samples == 0) return refuse(ctx, what, "width, height or samples is 0");
    if (int rc = pixels_check(ctx, what, (uint64_t)b->width * b->height)) return rc;
    if (!std::isfinite(b->probe_offset) || !(b->probe_offset > 0.0f)) return refuse(ctx, what, "probe_offset is not finite or not above 0");
    return CRT_OK;
}

static bool capturing(hipStream_t stream) {
    hipStreamCaptureStatus s = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(stream, &s) == hipSuccess && s != hipStreamCaptureStatusNone;
}

// The mesh's triangle list, made on first use: the trees are read back once (they are what says which triangles a mesh consists of: a
// crt_mesh is a tree root), the mesh's subtree is walked along its links, and what its leaves list is sorted and made unique.
static int bake_mesh(crt_ctx *ctx, const char *what, const uint32_t mesh, hipStream_t stream, BakeMesh **out) {
    crt_bake_state *B = ctx->bake;
    const SceneArgs &S = ctx->scene;
    if (B->meshes.size() == S.n_meshes && B->meshes[mesh]) {
        *out = B->meshes[mesh].get();
        return CRT_OK;
    }
    if (capturing(stream))
        return refuse(ctx, what, "the stream is being captured and mesh " + std::to_string(mesh) +
                                     "'s triangle list does not exist yet (it is read back and allocated by the first call for a mesh, outside a capture)");
    if (!B->trees) {
        B->nodes.resize(S.n_nodes);
        B->leaf_tris.resize(S.n_leaf_tris);
        B->mesh_recs.resize(S.n_meshes);
        if (S.n_nodes) CRT_HIP_CHECK(ctx, hipMemcpy(B->nodes.data(), S.nodes, (size_t)S.n_nodes * sizeof(crt_node), hipMemcpyDeviceToHost));
        if (S.n_leaf_tris) CRT_HIP_CHECK(ctx, hipMemcpy(B->leaf_tris.data(), S.leaf_tris, (size_t)S.n_leaf_tris * sizeof(uint32_t), hipMemcpyDeviceToHost));
        CRT_HIP_CHECK(ctx, hipMemcpy(B->mesh_recs.data(), S.meshes, (size_t)S.n_meshes * sizeof(crt_mesh), hipMemcpyDeviceToHost));
        B->meshes.resize(S.n_meshes);
        B->trees = true;
    }
    std::vector<uint32_t> tris;
    const uint32_t root = B->mesh_recs[mesh].root;
    if (root < S.n_nodes) {
        const uint32_t end = B->nodes[root].miss;
        // links and misses point to higher indices (crt_create checks it), so this ends
        for (uint32_t i = root; i != END && i != end && i < S.n_nodes;) {
            const crt_node &n = B->nodes[i];
            if (!is_leaf_link(n.link)) {
                i = n.link == END ? n.miss : n.link;
                continue;
            }
            for (uint64_t e = n.link & ~LEAF; e < S.n_leaf_tris; e++) {
                const uint32_t t = B->leaf_tris[e] & ~LAST;
                if (t < S.n_triangles) tris.push_back(t);
                if (B->leaf_tris[e] & LAST) break;
            }
            i = n.miss;
        }
    }
    std::sort(tris.begin(), tris.end());
    tris.erase(std::unique(tris.begin(), tris.end()), tris.end());
    std::unique_ptr<BakeMesh> M(new (std::nothrow) BakeMesh);
    if (!M) { ctx->error = "out of memory"; return CRT_ERR_NOMEM; }
    M->n = (uint32_t)tris.size();
    if (int rc = reserve_all(ctx, M->tris, std::max<uint64_t>(M->n, 1), M->large, (uint64_t)M->n + 1)) return rc;
    if (M->n) CRT_HIP_CHECK(ctx, hipMemcpy(M->tris.p, tris.data(), (size_t)M->n * sizeof(uint32_t), hipMemcpyHostToDevice));
    B->meshes[mesh] = std::move(M);
    *out = B->meshes[mesh].get();
    return CRT_OK;
}

static uint32_t blocks_of(const uint64_t n) { return (uint32_t)((n + BLOCK - 1) / BLOCK); }

// the rasteriser and the records: `b` checked, d_texels aligned to 16; d_status: a status plane beside the records, or null
static int bake_raster(crt_ctx *ctx, const crt_bake *b, BakeMesh *M, crt_bake_texel *d_texels, crt_ray *d_rays, uint8_t *d_status, void *d_work,
                       hipStream_t stream) {
    const SceneArgs &S = ctx->scene;
    const uint64_t n = (uint64_t)b->width * b->height;
    BakeOwnerArgs O{};
    O.tris = M->tris.p; O.n_tris = M->n;
    O.tri_verts = S.tri_verts; O.vuvs = S.vuvs;
    O.width = (int32_t)b->width; O.height = (int32_t)b->height;
    O.owner = (uint32_t *)d_work;
    O.large = M->large.p;
    O.n_triangles = S.n_triangles;
    hipLaunchKernelGGL(bake_reset, dim3(std::min<uint32_t>(blocks_of(n), BAKE_LARGE_BLOCKS)), dim3(BLOCK), 0, stream, O.owner, n, O.large);
    CRT_HIP_CHECK(ctx, hipGetLastError());
    if (M->n) {
        hipLaunchKernelGGL(bake_owner, dim3((M->n + BAKE_WAVES - 1) / BAKE_WAVES), dim3(BLOCK), 0, stream, O);
        CRT_HIP_CHECK(ctx, hipGetLastError());
        hipLaunchKernelGGL(bake_owner_large, dim3(BAKE_LARGE_BLOCKS), dim3(BLOCK), 0, stream, O);
        CRT_HIP_CHECK(ctx, hipGetLastError());
    }
    BakeTexelsArgs T{};
    T.owner = O.owner; T.tri_verts = S.tri_verts; T.vuvs = S.vuvs; T.tris = S.tris;
    T.width = O.width; T.height = O.height;
    T.tiles_x = tiles_x_of(b->width);
    T.mesh = b->mesh;
    T.n_triangles = S.n_triangles;
    T.probe_offset = b->probe_offset;
    T.texels = (float4 *)d_texels; T.rays = d_rays; T.status = d_status;
    hipLaunchKernelGGL(bake_texels, dim3(T.tiles_x * tiles_y_of(b->height)), dim3(TILE_X, TILE_Y), 0, stream, T);
    CRT_HIP_CHECK(ctx, hipGetLastError());
    return CRT_OK;
}

extern "C" int crt_bake_texels_device(crt_ctx *ctx, const crt_bake *bake, crt_bake_texel *d_texels, crt_ray *d_rays, void *d_work, void *stream) {
    const char *what = "crt_bake_texels_device";
    if (!ctx) return CRT_ERR_INVALID;
    if (int rc = bake_check(ctx, what, bake)) return rc;
    if (!d_texels || !d_rays || !d_work) return refuse(ctx, what, "d_texels, d_rays or d_work is NULL");
    if ((uintptr_t)d_texels % 16u || (uintptr_t)d_work % 16u) return refuse(ctx, what, "d_texels and d_work must be aligned to 16 bytes");
    if (ctx->pending) {
        if (capturing((hipStream_t)stream)) return refuse(ctx, what, "the stream is being captured and a crt_render_async frame is pending");
        if (int rc = crt_wait(ctx)) return rc;
    }
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (int rc = bake_state(ctx)) return rc;
    BakeMesh *M = nullptr;
    if (int rc = bake_mesh(ctx, what, bake->mesh, (hipStream_t)stream, &M)) return rc;
    return bake_raster(ctx, bake, M, d_texels, d_rays, nullptr, d_work, (hipStream_t)stream);
}

// `passes` dilation passes, ping-pong between the caller's map and the work area; the result ends in the caller's map
static int bake_dilate_run(crt_ctx *ctx, uint32_t width, uint32_t height, uint32_t passes, float *d_rgb, uint8_t *d_status, void *d_work, hipStream_t stream) {
    const uint64_t n = (uint64_t)width * height;
    passes = crt_bake_dilate_passes(width, height, passes);
    float *rgb[2] = {d_rgb, (float *)d_work};
    uint8_t *status[2] = {d_status, (uint8_t *)d_work + align16(12 * n)};
    BakeDilateArgs D{};
    D.width = (int32_t)width; D.height = (int32_t)height;
    D.tiles_x = tiles_x_of(width);
    const uint32_t grid = D.tiles_x * tiles_y_of(height);
    for (uint32_t k = 0; k < passes; k++) {
        D.rgb = rgb[k & 1]; D.status = status[k & 1];
        D.out_rgb = rgb[(k + 1) & 1]; D.out_status = status[(k + 1) & 1];
        hipLaunchKernelGGL(bake_dilate, dim3(grid), dim3(TILE_X, TILE_Y), 0, stream, D);
        CRT_HIP_CHECK(ctx, hipGetLastError());
    }
    if (passes & 1u) {
        // (kernels, not copy nodes: a captured call is a chain of kernel nodes)
        hipLaunchKernelGGL(bake_copy, dim3(std::min<uint32_t>(blocks_of(12 * n), BAKE_LARGE_BLOCKS)), dim3(BLOCK), 0, stream, (const uint8_t *)rgb[1], (uint8_t *)d_rgb, 12 * n);
        hipLaunchKernelGGL(bake_copy, dim3(std::min<uint32_t>(blocks_of(n), BAKE_LARGE_BLOCKS)), dim3(BLOCK), 0, stream, (const uint8_t *)status[1], d_status, n);
        CRT_HIP_CHECK(ctx, hipGetLastError());
    }
    return CRT_OK;
}

extern "C" int crt_bake_dilate_device(crt_ctx *ctx, uint32_t width, uint32_t height, uint32_t passes, float *d_rgb, uint8_t *d_status, void *d_work,
                                      void *stream) {
    const char *what = "crt_bake_dilate_device";
    if (!ctx) return CRT_ERR_INVALID;
    if (width == 0 || height == 0) return refuse(ctx, what, "width or height is 0");
    if (int rc = pixels_check(ctx, what, (uint64_t)width * height)) return rc;
    if (!d_rgb || !d_status || !d_work) return refuse(ctx, what, "d_rgb, d_status or d_work is NULL");
    if ((uintptr_t)d_work % 16u) return refuse(ctx, what, "d_work must be aligned to 16 bytes");
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    return bake_dilate_run(ctx, width, height, passes, d_rgb, d_status, d_work, (hipStream_t)stream);
}

extern "C" int crt_bake_lightmap(crt_ctx *ctx, const crt_bake *bake, const crt_options *options, float *out_rgb, uint8_t *out_rgb8, uint8_t *out_status,
                                 crt_bake_texel *out_texels) {
    const char *what = "crt_bake_lightmap";
    if (!ctx) return CRT_ERR_INVALID;
    if (int rc = bake_check(ctx, what, bake)) return rc;
    if (!options) return refuse(ctx, what, "options is NULL");
    // what the radiance call behind it would refuse, asked before anything is enqueued
    const bool gi = options->use_gi != 0;
    if (int rc = query_shoot_check(ctx, what, options)) return rc;
    if (ctx->pending)
        if (int rc = crt_wait(ctx)) return rc;
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (int rc = bake_state(ctx)) return rc;
    crt_bake_state *B = ctx->bake;
    hipStream_t stream = ctx->stream;
    BakeMesh *M = nullptr;
    if (int rc = bake_mesh(ctx, what, bake->mesh, stream, &M)) return rc;
    const uint32_t W = bake->width, H = bake->height;
    const uint64_t n = (uint64_t)W * H;
    const uint32_t blocks = blocks_of(n);
    if (int rc = reserve_all(ctx, B->texels, 3 * n, B->work, float4s(crt_bake_work_bytes(W, H)), B->rays, n, B->status, n, B->map, 3 * n, B->counts,
                             (uint64_t)COUNT_WORDS, B->list_work, (uint64_t)blocks * BAKE_WAVES + blocks))
        return rc;
    if (!B->pin) CRT_HIP_CHECK(ctx, hipHostMalloc((void **)&B->pin, COUNT_WORDS * sizeof(uint32_t)));
    for (hipEvent_t &e : B->ev)
        if (!e) CRT_HIP_CHECK(ctx, hipEventCreate(&e));

    // 1. rasterise, and count the covered texels
    CRT_HIP_CHECK(ctx, hipEventRecord(B->ev[0], stream));
    CRT_HIP_CHECK(ctx, hipMemsetAsync(B->counts.p, 0, COUNT_WORDS * sizeof(uint32_t), stream));
    if (int rc = bake_raster(ctx, bake, M, (crt_bake_texel *)B->texels.p, B->rays.p, B->status.p, B->work.p, stream)) return rc;
    BakeListWork LW{B->list_work.p, (uint32_t *)(B->list_work.p + (uint64_t)blocks * BAKE_WAVES), nullptr};
    LW.offsets = LW.counts + blocks;   // (blocks unsigned long longs hold 2 * blocks words)
    hipLaunchKernelGGL(bake_mark, dim3(blocks), dim3(BLOCK), 0, stream, BakeMarkArgs{B->status.p, n, LW});
    CRT_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(bake_scan, dim3(1), dim3(BLOCK), 0, stream, BakeScanArgs{LW.counts, LW.offsets, B->counts.p + COUNT_COVERED, blocks});
    CRT_HIP_CHECK(ctx, hipGetLastError());
    // 2. the one count the host needs
    CRT_HIP_CHECK(ctx, hipMemcpyAsync(B->pin, B->counts.p, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    CRT_HIP_CHECK(ctx, hipStreamSynchronize(stream));
    const uint64_t covered = B->pin[COUNT_COVERED];
    if (covered > n) { ctx->error = std::string(what) + ": the covered texels' count is larger than the map"; return CRT_ERR_HIP; }
    if (int rc = reserve_all(ctx, B->list, std::max<uint64_t>(covered, 1), B->list_rays, std::max<uint64_t>(covered, 1), B->rgb,
                             3 * std::max<uint64_t>(covered, 1)))
        return rc;
    if (gi)
        if (int rc = reserve_all(ctx, B->keys, std::max<uint64_t>(covered, 1), B->sum, 3 * n)) return rc;
    if (bake->check_probes)
        if (int rc = B->hits.reserve(ctx, std::max<uint64_t>(covered, 1))) return rc;
    if (out_rgb8)
        if (int rc = B->q8.reserve(ctx, 3 * n)) return rc;
    hipLaunchKernelGGL(bake_scatter, dim3(blocks), dim3(BLOCK), 0, stream, BakeScatterArgs{n, LW, B->rays.p, B->list.p, B->list_rays.p});
    CRT_HIP_CHECK(ctx, hipGetLastError());
    CRT_HIP_CHECK(ctx, hipMemsetAsync(B->map.p, 0, 12 * n, stream));
    CRT_HIP_CHECK(ctx, hipEventRecord(B->ev[1], stream));

    // 3. shoot the list and 4. scatter it to the map (EMPTY texels stay 0)
    if (covered) {
        BakeFoldArgs F{};
        F.rgb = B->rgb.p; F.list = B->list.p;
        F.n = covered; F.map_texels = n;
        F.map = B->map.p;
        if (!gi) {
            if (int rc = crt_shoot_rays_device(ctx, B->list_rays.p, covered, CRT_RAY_REFLECTION, options, B->rgb.p, stream)) return rc;
            hipLaunchKernelGGL(bake_fold, dim3(blocks_of(covered)), dim3(BLOCK), 0, stream, F);
            CRT_HIP_CHECK(ctx, hipGetLastError());
        } else {
            F.sum = B->sum.p;
            for (uint32_t s = 0; s < bake->samples; s++) {
                hipLaunchKernelGGL(bake_keys, dim3(blocks_of(covered)), dim3(BLOCK), 0, stream, BakeKeysArgs{B->list.p, covered, options->gi_seed, s, B->keys.p});
                CRT_HIP_CHECK(ctx, hipGetLastError());
                if (int rc = crt_shoot_rays_gi_device(ctx, B->list_rays.p, B->keys.p, covered, CRT_RAY_REFLECTION, options, B->rgb.p, stream)) return rc;
                F.sample = s;
                hipLaunchKernelGGL(bake_fold, dim3(blocks_of(covered)), dim3(BLOCK), 0, stream, F);
                CRT_HIP_CHECK(ctx, hipGetLastError());
            }
        }
        if (bake->check_probes) {
            if (int rc = crt_trace_rays_device(ctx, B->list_rays.p, covered, CRT_RAY_REFLECTION, B->hits.p, stream)) return rc;
            hipLaunchKernelGGL(bake_count_self, dim3(blocks_of(covered)), dim3(BLOCK), 0, stream, B->hits.p, B->list.p, B->texels.p, covered,
                               B->counts.p + COUNT_SELF);
            CRT_HIP_CHECK(ctx, hipGetLastError());
        }
    }
    CRT_HIP_CHECK(ctx, hipEventRecord(B->ev[2], stream));

    // 5. dilate and 6. quantise
    if (int rc = bake_dilate_run(ctx, W, H, bake->dilate, B->map.p, B->status.p, B->work.p, stream)) return rc;
    hipLaunchKernelGGL(bake_count_status, dim3(blocks), dim3(BLOCK), 0, stream, B->status.p, n, (uint8_t)CRT_BAKE_STATUS_DILATED, B->counts.p + COUNT_DILATED);
    CRT_HIP_CHECK(ctx, hipGetLastError());
    if (out_rgb8) {
        if (int rc = crt_quantize_device(ctx, B->map.p, 3 * n, B->q8.p, stream)) return rc;
        CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_rgb8, B->q8.p, 3 * n, hipMemcpyDeviceToHost, stream));
    }
    if (out_rgb) CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_rgb, B->map.p, 12 * n, hipMemcpyDeviceToHost, stream));
    if (out_status) CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_status, B->status.p, n, hipMemcpyDeviceToHost, stream));
    if (out_texels) CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_texels, B->texels.p, 48 * n, hipMemcpyDeviceToHost, stream));
    CRT_HIP_CHECK(ctx, hipMemcpyAsync(B->pin, B->counts.p, COUNT_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    CRT_HIP_CHECK(ctx, hipEventRecord(B->ev[3], stream));
    CRT_HIP_CHECK(ctx, hipStreamSynchronize(stream));

    crt_bake_stats &st = B->stats;
    st = crt_bake_stats{};
    st.texels = n;
    st.covered = covered;
    st.dilated = B->pin[COUNT_DILATED];
    st.probe_self = bake->check_probes ? B->pin[COUNT_SELF] : 0;
    float ms = 0;
    CRT_HIP_CHECK(ctx, hipEventElapsedTime(&ms, B->ev[0], B->ev[1]));
    st.raster_ms = ms;
    CRT_HIP_CHECK(ctx, hipEventElapsedTime(&ms, B->ev[1], B->ev[2]));
    st.shoot_ms = ms;
    CRT_HIP_CHECK(ctx, hipEventElapsedTime(&ms, B->ev[0], B->ev[3]));
    st.total_ms = ms;
    return CRT_OK;
}

extern "C" int crt_get_bake_stats(crt_ctx *ctx, crt_bake_stats *out) {
    if (!ctx || !out) return CRT_ERR_INVALID;
    *out = ctx->bake ? ctx->bake->stats : crt_bake_stats{};
    return CRT_OK;
}
