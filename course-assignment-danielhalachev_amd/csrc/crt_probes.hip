// crt_probes.hip -- the irradiance probe volume (include/crt_hip.h: "Irradiance probes"): crt_probe_volume_defaults, the four enqueue-only
// primitives crt_probe_rays_device, crt_probe_project_device, crt_probe_validity_device and crt_probe_irradiance_device, the synchronous
// crt_bake_probes and crt_probe_irradiance, and crt_get_probe_stats.  Kernels: csrc/kernel_probes.h; the rule: csrc/probe_rule.h.  The
// colours are the radiance queries' (crt_shoot_rays_device, crt_shoot_rays_gi_device) and the hits crt_trace_rays_device's, called as any
// caller calls them; nothing of a frame, a walk, a query or a lightmap bake is touched.  And the volume's visibility term (include/crt_hip.h:
// "Probe visibility"): crt_probe_visibility_defaults, the enqueue-only crt_probe_depth_device and crt_probe_irradiance_visible_device, the
// synchronous crt_bake_probes_visible -- crt_bake_probes' chunk loop with one trace a chunk for the validity and the depth pass -- and
// crt_probe_irradiance_visible.  Kernels: csrc/kernel_probe_depth.h; the rule: csrc/probe_depth_rule.h.  And the picture that reads the volume
// (include/crt_hip.h: "Probe-lit radiance"): the enqueue-only crt_probe_light_hits_device, crt_shoot_rays_lit* -- crt_query.hip's GI level loop
// with that launch behind every level's lighting --, crt_render_probe_lit and crt_get_probe_lit_stats.  Kernel: csrc/kernel_probe_light.h; the
// rule: csrc/probe_lit_rule.h.
#include "crt_internal.h"
#include "device_array.h"

namespace {
#include "kernel_probes.h"
#include "kernel_probe_depth.h"
#include "kernel_probe_light.h"
}  // namespace

static_assert(sizeof(crt_probe_volume) == 48 && sizeof(crt_probe_grid) == 48 && offsetof(crt_probe_volume, nx) == offsetof(crt_probe_grid, n) &&
                  offsetof(crt_probe_volume, rays) == offsetof(crt_probe_grid, rays) && offsetof(crt_probe_volume, gi_seed) == offsetof(crt_probe_grid, gi_seed) &&
                  offsetof(crt_probe_volume, backface_limit) == offsetof(crt_probe_grid, backface_limit),
              "the rule reads crt_probe_volume as it is");
static_assert(sizeof(crt_probe) == 128 && offsetof(crt_probe, rays) == 4 * CRT_PROBE_WORD_RAYS && offsetof(crt_probe, back) == 4 * CRT_PROBE_WORD_BACK &&
                  offsetof(crt_probe, miss) == 4 * CRT_PROBE_WORD_MISS && offsetof(crt_probe, state) == 4 * CRT_PROBE_WORD_STATE &&
                  offsetof(crt_probe, pad) == 4 * CRT_PROBE_WORD_PAD,
              "a record is eight 16-byte stores, the state in the last");
static_assert(CRT_PROBE_INVALID == CRT_PROBE_STATE_INVALID && CRT_PROBE_VALID == CRT_PROBE_STATE_VALID, "the rule's states are the header's");
static_assert(sizeof(crt_ray) == 24 && sizeof(crt_hit) == 48, "a ray is a 16-byte and an 8-byte store");
static_assert(sizeof(crt_probe_depth) == 512 && sizeof(crt_probe_depth) == CRT_PROBE_DEPTH_TEXELS * sizeof(float2), "a depth record is a wave's 64 8-byte stores");
static_assert(sizeof(crt_probe_visibility) == 20 && sizeof(crt_probe_vis) == 20 && offsetof(crt_probe_visibility, max_distance) == offsetof(crt_probe_vis, max_distance) &&
                  offsetof(crt_probe_visibility, min_weight) == offsetof(crt_probe_vis, min_weight),
              "the rule reads crt_probe_visibility as it is");

// rays of one chunk of crt_bake_probes: its scratch is 88 bytes a ray (ray, key, colour, hit)
constexpr uint64_t PROBE_CHUNK_RAYS = 1ull << 20;

struct crt_probe_state {
    // crt_bake_probes: one chunk's rays, keys, colours and hits, the records when the caller keeps none on the device, the invalid count
    DeviceArray<crt_ray> rays;
    DeviceArray<uint32_t> keys, counts;
    DeviceArray<float> rgb;
    DeviceArray<crt_hit> hits;
    DeviceArray<float4> probes;
    DeviceArray<float2> depth;   // crt_bake_probes_visible: the depth records when the caller keeps none on the device
    // crt_probe_irradiance and crt_probe_irradiance_visible: the volume's records, the points, the normals, the colours, the statuses
    DeviceArray<float4> look_probes;
    DeviceArray<float2> look_depth;
    DeviceArray<float> points, normals, look_rgb;
    DeviceArray<uint8_t> status;
    // crt_shoot_rays_lit* and crt_render_probe_lit: the host variant's and the frame's rays, the call's LIT and UNLIT counters, their pinned
    // copy, and the event behind that copy (lit_open: it has not been read yet)
    DeviceArray<crt_ray> lit_rays;
    DeviceArray<unsigned long long> lit_counts;
    unsigned long long *lit_pin = nullptr;
    hipEvent_t lit_ev = nullptr;
    bool lit_open = false;
    crt_probe_lit_stats lit_stats{};
    uint32_t *pin = nullptr;
    hipEvent_t ev[4] = {};
    crt_probe_stats stats{};
    ~crt_probe_state() {
        if (lit_pin) (void)hipHostFree(lit_pin);
        if (lit_ev) (void)hipEventDestroy(lit_ev);
        if (pin) (void)hipHostFree(pin);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

void probes_destroy(crt_ctx *ctx) {
    delete ctx->probes;
    ctx->probes = nullptr;
}

static int probes_state(crt_ctx *ctx) {
    if (!ctx->probes) ctx->probes = new (std::nothrow) crt_probe_state;
    if (!ctx->probes) { ctx->error = "out of memory"; return CRT_ERR_NOMEM; }
    return CRT_OK;
}

extern "C" void crt_probe_volume_defaults(crt_probe_volume *v) {
    if (!v) return;
    for (int k = 0; k < 3; k++) { v->origin[k] = 0.0f; v->spacing[k] = 1.0f; }
    v->nx = v->ny = v->nz = 1;
    v->rays = 64;
    v->gi_seed = 0;
    v->backface_limit = 1.0f;
}

static crt_probe_grid grid_of(const crt_probe_volume *v) {
    crt_probe_grid g;
    memcpy(&g, v, sizeof(g));
    return g;
}

static int volume_check(crt_ctx *ctx, const char *what, const crt_probe_volume *v) {
    if (!v) return refuse(ctx, what, "volume is NULL");
    if (!crt_probe_grid_valid(grid_of(v)))
        return refuse(ctx, what, "the volume is not valid: nx, ny, nz >= 1, 1 <= rays <= 4096, nx * ny * nz < 2^24, finite origin, spacing finite and > 0, "
                                 "backface_limit finite in [0, 1]");
    return CRT_OK;
}

static uint32_t blocks_of(const uint64_t n) { return (uint32_t)((n + BLOCK - 1) / BLOCK); }
static uint32_t wave_blocks_of(const uint64_t waves) { return (uint32_t)((waves + PROBE_WAVES - 1) / PROBE_WAVES); }

// what the two per-probe primitives ask of (count, rays): count * rays rays in arrays of the caller's
static int range_check(crt_ctx *ctx, const char *what, const uint64_t count, const uint32_t rays) {
    if (rays == 0u || rays > CRT_PROBE_MAX_RAYS) return refuse(ctx, what, "rays = " + std::to_string(rays) + " is not in 1 .. 4096");
    if (count >= CRT_PROBE_MAX_PROBES) return refuse(ctx, what, "count = " + std::to_string(count) + " >= 2^24");
    return CRT_OK;
}

extern "C" int crt_probe_rays_device(crt_ctx *ctx, const crt_probe_volume *volume, uint32_t first, uint32_t count, crt_ray *d_rays, uint32_t *d_keys,
                                     void *stream) {
    const char *what = "crt_probe_rays_device";
    if (!ctx) return CRT_ERR_INVALID;
    if (int rc = volume_check(ctx, what, volume)) return rc;
    const crt_probe_grid g = grid_of(volume);
    if ((uint64_t)first + count > crt_probe_count(g))
        return refuse(ctx, what, "first + count = " + std::to_string((uint64_t)first + count) + " > the volume's " + std::to_string(crt_probe_count(g)) + " probes");
    if (count == 0) return CRT_OK;
    if (!d_rays) return refuse(ctx, what, "d_rays is NULL");
    if ((uintptr_t)d_rays % 16u) return refuse(ctx, what, "d_rays must be aligned to 16 bytes");
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(probe_rays, dim3(blocks_of((uint64_t)count * g.rays)), dim3(BLOCK), 0, (hipStream_t)stream, ProbeRaysArgs{g, first, count, d_rays, d_keys});
    CRT_HIP_CHECK(ctx, hipGetLastError());
    return CRT_OK;
}

extern "C" int crt_probe_project_device(crt_ctx *ctx, const crt_ray *d_rays, const float *d_rgb, uint32_t count, uint32_t rays, crt_probe *d_probes,
                                        void *stream) {
    const char *what = "crt_probe_project_device";
    if (!ctx) return CRT_ERR_INVALID;
    if (int rc = range_check(ctx, what, count, rays)) return rc;
    if (count == 0) return CRT_OK;
    if (!d_rays || !d_rgb || !d_probes) return refuse(ctx, what, "d_rays, d_rgb or d_probes is NULL");
    if ((uintptr_t)d_probes % 16u) return refuse(ctx, what, "d_probes must be aligned to 16 bytes");
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(probe_project, dim3(wave_blocks_of(count)), dim3(BLOCK), 0, (hipStream_t)stream, ProbeProjectArgs{d_rays, d_rgb, count, rays, (float4 *)d_probes});
    CRT_HIP_CHECK(ctx, hipGetLastError());
    return CRT_OK;
}

extern "C" int crt_probe_validity_device(crt_ctx *ctx, const crt_ray *d_rays, const crt_hit *d_hits, uint32_t count, uint32_t rays, float backface_limit,
                                         crt_probe *d_probes, void *stream) {
    const char *what = "crt_probe_validity_device";
    if (!ctx) return CRT_ERR_INVALID;
    if (int rc = range_check(ctx, what, count, rays)) return rc;
    if (!crt_finite(backface_limit) || !(backface_limit >= 0.0f && backface_limit <= 1.0f)) return refuse(ctx, what, "backface_limit is not finite in [0, 1]");
    if (count == 0) return CRT_OK;
    if (!d_rays || !d_hits || !d_probes) return refuse(ctx, what, "d_rays, d_hits or d_probes is NULL");
    if ((uintptr_t)d_probes % 16u) return refuse(ctx, what, "d_probes must be aligned to 16 bytes");
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(probe_validity, dim3(wave_blocks_of(count)), dim3(BLOCK), 0, (hipStream_t)stream,
                       ProbeValidityArgs{d_rays, d_hits, count, rays, backface_limit, (float4 *)d_probes});
    CRT_HIP_CHECK(ctx, hipGetLastError());
    return CRT_OK;
}

extern "C" int crt_probe_irradiance_device(crt_ctx *ctx, const crt_probe_volume *volume, const crt_probe *d_probes, const float *d_points,
                                           const float *d_normals, uint64_t n, float *d_rgb, uint8_t *d_status, void *stream) {
    const char *what = "crt_probe_irradiance_device";
    if (!ctx) return CRT_ERR_INVALID;
    if (int rc = volume_check(ctx, what, volume)) return rc;
    if (n == 0) return CRT_OK;
    if (n >= CRT_MAX_PIXELS) return refuse(ctx, what, "n = " + std::to_string(n) + " >= 2^31");
    if (!d_probes || !d_points || !d_normals || !d_rgb) return refuse(ctx, what, "d_probes, d_points, d_normals or d_rgb is NULL");
    if ((uintptr_t)d_probes % 16u) return refuse(ctx, what, "d_probes must be aligned to 16 bytes");
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(probe_lookup, dim3(blocks_of(n)), dim3(BLOCK), 0, (hipStream_t)stream,
                       ProbeLookupArgs{grid_of(volume), (const float4 *)d_probes, d_points, d_normals, n, d_rgb, d_status});
    CRT_HIP_CHECK(ctx, hipGetLastError());
    return CRT_OK;
}

static crt_probe_vis vis_of(const crt_probe_visibility *v) {
    crt_probe_vis p;
    memcpy(&p, v, sizeof(p));
    return p;
}

static int visibility_check(crt_ctx *ctx, const char *what, const crt_probe_visibility *v) {
    if (!v) return refuse(ctx, what, "visibility is NULL");
    if (!crt_probe_vis_valid(vis_of(v)))
        return refuse(ctx, what, "the visibility is not valid: size == sizeof(crt_probe_visibility), max_distance finite and > 0, normal_bias finite and >= 0, "
                                 "variance_floor finite and > 0, min_weight finite in (0, 1]");
    return CRT_OK;
}

extern "C" int crt_probe_visibility_defaults(const crt_probe_volume *volume, crt_probe_visibility *visibility) {
    if (!volume || !visibility || !crt_probe_grid_valid(grid_of(volume))) return CRT_ERR_INVALID;
    crt_probe_vis p;
    crt_probe_vis_defaults(grid_of(volume), &p);
    memcpy(visibility, &p, sizeof(p));
    return CRT_OK;
}

extern "C" int crt_probe_depth_device(crt_ctx *ctx, const crt_ray *d_rays, const crt_hit *d_hits, uint32_t count, uint32_t rays, float max_distance,
                                      crt_probe_depth *d_depth, void *stream) {
    const char *what = "crt_probe_depth_device";
    if (!ctx) return CRT_ERR_INVALID;
    if (int rc = range_check(ctx, what, count, rays)) return rc;
    if (!crt_finite(max_distance) || !(max_distance > 0.0f)) return refuse(ctx, what, "max_distance is not finite and > 0");
    if (count == 0) return CRT_OK;
    if (!d_rays || !d_hits || !d_depth) return refuse(ctx, what, "d_rays, d_hits or d_depth is NULL");
    if ((uintptr_t)d_depth % 16u) return refuse(ctx, what, "d_depth must be aligned to 16 bytes");
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(probe_depth, dim3(wave_blocks_of(count)), dim3(BLOCK), 0, (hipStream_t)stream,
                       ProbeDepthArgs{d_rays, d_hits, count, rays, max_distance, (float2 *)d_depth});
    CRT_HIP_CHECK(ctx, hipGetLastError());
    return CRT_OK;
}

extern "C" int crt_probe_irradiance_visible_device(crt_ctx *ctx, const crt_probe_volume *volume, const crt_probe_visibility *visibility, const crt_probe *d_probes,
                                                   const crt_probe_depth *d_depth, const float *d_points, const float *d_normals, uint64_t n, float *d_rgb,
                                                   uint8_t *d_status, void *stream) {
    const char *what = "crt_probe_irradiance_visible_device";
    if (!ctx) return CRT_ERR_INVALID;
    if (int rc = volume_check(ctx, what, volume)) return rc;
    if (int rc = visibility_check(ctx, what, visibility)) return rc;
    if (n == 0) return CRT_OK;
    if (n >= CRT_MAX_PIXELS) return refuse(ctx, what, "n = " + std::to_string(n) + " >= 2^31");
    if (!d_probes || !d_depth || !d_points || !d_normals || !d_rgb) return refuse(ctx, what, "d_probes, d_depth, d_points, d_normals or d_rgb is NULL");
    if ((uintptr_t)d_probes % 16u || (uintptr_t)d_depth % 16u) return refuse(ctx, what, "d_probes and d_depth must be aligned to 16 bytes");
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(probe_lookup_visible, dim3(blocks_of(n)), dim3(BLOCK), 0, (hipStream_t)stream,
                       ProbeLookupVisibleArgs{grid_of(volume), vis_of(visibility), (const float4 *)d_probes, (const float2 *)d_depth, d_points, d_normals, n, d_rgb,
                                              d_status});
    CRT_HIP_CHECK(ctx, hipGetLastError());
    return CRT_OK;
}

// crt_bake_probes (visibility == NULL: no depth pass, the trace only for the validity pass) and crt_bake_probes_visible
static int bake_probes(crt_ctx *ctx, const char *what, const crt_probe_volume *volume, const crt_probe_visibility *visibility, const crt_options *options,
                       crt_probe *out_probes, crt_probe *d_probes, crt_probe_depth *out_depth, crt_probe_depth *d_depth) {
    if (!ctx) return CRT_ERR_INVALID;
    if (int rc = volume_check(ctx, what, volume)) return rc;
    if (visibility)
        if (int rc = visibility_check(ctx, what, visibility)) return rc;
    if (!options) return refuse(ctx, what, "options is NULL");
    if (d_probes && (uintptr_t)d_probes % 16u) return refuse(ctx, what, "d_probes must be aligned to 16 bytes");
    if (d_depth && (uintptr_t)d_depth % 16u) return refuse(ctx, what, "d_depth must be aligned to 16 bytes");
    // what the radiance call behind it would refuse, asked before anything is enqueued
    if (int rc = query_shoot_check(ctx, what, options)) return rc;
    if (ctx->pending)
        if (int rc = crt_wait(ctx)) return rc;
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (int rc = probes_state(ctx)) return rc;
    crt_probe_state *B = ctx->probes;
    hipStream_t stream = ctx->stream;
    const crt_probe_grid g = grid_of(volume);
    const uint32_t total = crt_probe_count(g), R = g.rays;
    const bool gi = options->use_gi != 0, validity = g.backface_limit != 1.0f, depth = visibility != nullptr;
    const uint32_t chunk = ctx->probe_chunk ? ctx->probe_chunk : (uint32_t)std::max<uint64_t>(PROBE_CHUNK_RAYS / R, 1u);
    const uint64_t chunk_rays = (uint64_t)std::min(chunk, total) * R;
    if (int rc = reserve_all(ctx, B->rays, chunk_rays, B->rgb, 3 * chunk_rays, B->counts, (uint64_t)1)) return rc;
    if (gi)
        if (int rc = B->keys.reserve(ctx, chunk_rays)) return rc;
    if (validity || depth)
        if (int rc = B->hits.reserve(ctx, chunk_rays)) return rc;
    if (!d_probes)
        if (int rc = B->probes.reserve(ctx, 8 * (uint64_t)total)) return rc;
    if (depth && !d_depth)
        if (int rc = B->depth.reserve(ctx, CRT_PROBE_DEPTH_TEXELS * (uint64_t)total)) return rc;
    crt_probe *records = d_probes ? d_probes : (crt_probe *)B->probes.p;
    crt_probe_depth *maps = d_depth ? d_depth : (crt_probe_depth *)B->depth.p;
    if (!B->pin) CRT_HIP_CHECK(ctx, hipHostMalloc((void **)&B->pin, sizeof(uint32_t)));
    for (hipEvent_t &e : B->ev)
        if (!e) CRT_HIP_CHECK(ctx, hipEventCreate(&e));

    double shoot_ms = 0, project_ms = 0, total_ms = 0;
    for (uint32_t first = 0; first < total; first += chunk) {
        const uint32_t count = std::min(chunk, total - first);
        const uint64_t n = (uint64_t)count * R;
        CRT_HIP_CHECK(ctx, hipEventRecord(B->ev[0], stream));
        if (int rc = crt_probe_rays_device(ctx, volume, first, count, B->rays.p, gi ? B->keys.p : nullptr, stream)) return rc;
        CRT_HIP_CHECK(ctx, hipEventRecord(B->ev[1], stream));
        if (int rc = gi ? crt_shoot_rays_gi_device(ctx, B->rays.p, B->keys.p, n, CRT_RAY_REFLECTION, options, B->rgb.p, stream)
                        : crt_shoot_rays_device(ctx, B->rays.p, n, CRT_RAY_REFLECTION, options, B->rgb.p, stream))
            return rc;
        CRT_HIP_CHECK(ctx, hipEventRecord(B->ev[2], stream));
        if (int rc = crt_probe_project_device(ctx, B->rays.p, B->rgb.p, count, R, records + first, stream)) return rc;
        if (validity || depth)   // one trace serves both passes
            if (int rc = crt_trace_rays_device(ctx, B->rays.p, n, CRT_RAY_REFLECTION, B->hits.p, stream)) return rc;
        if (validity)
            if (int rc = crt_probe_validity_device(ctx, B->rays.p, B->hits.p, count, R, g.backface_limit, records + first, stream)) return rc;
        if (depth)
            if (int rc = crt_probe_depth_device(ctx, B->rays.p, B->hits.p, count, R, visibility->max_distance, maps + first, stream)) return rc;
        CRT_HIP_CHECK(ctx, hipEventRecord(B->ev[3], stream));
        CRT_HIP_CHECK(ctx, hipStreamSynchronize(stream));   // the next chunk writes the same scratch, and the events are read
        float ms = 0;
        CRT_HIP_CHECK(ctx, hipEventElapsedTime(&ms, B->ev[1], B->ev[2]));
        shoot_ms += ms;
        CRT_HIP_CHECK(ctx, hipEventElapsedTime(&ms, B->ev[2], B->ev[3]));
        project_ms += ms;
        CRT_HIP_CHECK(ctx, hipEventElapsedTime(&ms, B->ev[0], B->ev[3]));
        total_ms += ms;
    }
    CRT_HIP_CHECK(ctx, hipMemsetAsync(B->counts.p, 0, sizeof(uint32_t), stream));
    hipLaunchKernelGGL(probe_count_invalid, dim3(blocks_of(total)), dim3(BLOCK), 0, stream, (const float4 *)records, (uint64_t)total, B->counts.p);
    CRT_HIP_CHECK(ctx, hipGetLastError());
    CRT_HIP_CHECK(ctx, hipMemcpyAsync(B->pin, B->counts.p, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    if (out_probes) CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_probes, records, (size_t)total * sizeof(crt_probe), hipMemcpyDeviceToHost, stream));
    if (depth && out_depth) CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_depth, maps, (size_t)total * sizeof(crt_probe_depth), hipMemcpyDeviceToHost, stream));
    CRT_HIP_CHECK(ctx, hipStreamSynchronize(stream));

    crt_probe_stats &st = B->stats;
    st = crt_probe_stats{};
    st.probes = total;
    st.invalid = B->pin[0];
    st.rays = (uint64_t)total * R;
    st.shoot_ms = shoot_ms;
    st.project_ms = project_ms;
    st.total_ms = total_ms;
    return CRT_OK;
}

extern "C" int crt_bake_probes(crt_ctx *ctx, const crt_probe_volume *volume, const crt_options *options, crt_probe *out_probes, crt_probe *d_probes) {
    return bake_probes(ctx, "crt_bake_probes", volume, nullptr, options, out_probes, d_probes, nullptr, nullptr);
}

extern "C" int crt_bake_probes_visible(crt_ctx *ctx, const crt_probe_volume *volume, const crt_probe_visibility *visibility, const crt_options *options,
                                       crt_probe *out_probes, crt_probe *d_probes, crt_probe_depth *out_depth, crt_probe_depth *d_depth) {
    const char *what = "crt_bake_probes_visible";
    if (!ctx) return CRT_ERR_INVALID;
    if (!visibility) return refuse(ctx, what, "visibility is NULL");
    return bake_probes(ctx, what, volume, visibility, options, out_probes, d_probes, out_depth, d_depth);
}

extern "C" int crt_probe_irradiance_visible(crt_ctx *ctx, const crt_probe_volume *volume, const crt_probe_visibility *visibility, const crt_probe *probes,
                                            const crt_probe_depth *depth, const float *points, const float *normals, uint64_t n, float *out_rgb,
                                            uint8_t *out_status) {
    const char *what = "crt_probe_irradiance_visible";
    if (!ctx) return CRT_ERR_INVALID;
    if (int rc = volume_check(ctx, what, volume)) return rc;
    if (int rc = visibility_check(ctx, what, visibility)) return rc;
    if (n == 0) return CRT_OK;
    if (n >= CRT_MAX_PIXELS) return refuse(ctx, what, "n = " + std::to_string(n) + " >= 2^31");
    if (!probes || !depth || !points || !normals || !out_rgb) return refuse(ctx, what, "probes, depth, points, normals or out_rgb is NULL");
    if (ctx->pending)
        if (int rc = crt_wait(ctx)) return rc;
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (int rc = probes_state(ctx)) return rc;
    crt_probe_state *B = ctx->probes;
    hipStream_t stream = ctx->stream;
    const uint64_t total = crt_probe_count(grid_of(volume));
    if (int rc = reserve_all(ctx, B->look_probes, 8 * total, B->look_depth, CRT_PROBE_DEPTH_TEXELS * total, B->points, 3 * n, B->normals, 3 * n, B->look_rgb, 3 * n,
                             B->status, n))
        return rc;
    CRT_HIP_CHECK(ctx, hipMemcpyAsync(B->look_probes.p, probes, (size_t)total * sizeof(crt_probe), hipMemcpyHostToDevice, stream));
    CRT_HIP_CHECK(ctx, hipMemcpyAsync(B->look_depth.p, depth, (size_t)total * sizeof(crt_probe_depth), hipMemcpyHostToDevice, stream));
    CRT_HIP_CHECK(ctx, hipMemcpyAsync(B->points.p, points, (size_t)n * 12, hipMemcpyHostToDevice, stream));
    CRT_HIP_CHECK(ctx, hipMemcpyAsync(B->normals.p, normals, (size_t)n * 12, hipMemcpyHostToDevice, stream));
    if (int rc = crt_probe_irradiance_visible_device(ctx, volume, visibility, (const crt_probe *)B->look_probes.p, (const crt_probe_depth *)B->look_depth.p,
                                                     B->points.p, B->normals.p, n, B->look_rgb.p, B->status.p, stream))
        return rc;
    CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_rgb, B->look_rgb.p, (size_t)n * 12, hipMemcpyDeviceToHost, stream));
    if (out_status) CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_status, B->status.p, (size_t)n, hipMemcpyDeviceToHost, stream));
    CRT_HIP_CHECK(ctx, hipStreamSynchronize(stream));
    return CRT_OK;
}

extern "C" int crt_probe_irradiance(crt_ctx *ctx, const crt_probe_volume *volume, const crt_probe *probes, const float *points, const float *normals,
                                    uint64_t n, float *out_rgb, uint8_t *out_status) {
    const char *what = "crt_probe_irradiance";
    if (!ctx) return CRT_ERR_INVALID;
    if (int rc = volume_check(ctx, what, volume)) return rc;
    if (n == 0) return CRT_OK;
    if (n >= CRT_MAX_PIXELS) return refuse(ctx, what, "n = " + std::to_string(n) + " >= 2^31");
    if (!probes || !points || !normals || !out_rgb) return refuse(ctx, what, "probes, points, normals or out_rgb is NULL");
    if (ctx->pending)
        if (int rc = crt_wait(ctx)) return rc;
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (int rc = probes_state(ctx)) return rc;
    crt_probe_state *B = ctx->probes;
    hipStream_t stream = ctx->stream;
    const uint64_t total = crt_probe_count(grid_of(volume));
    if (int rc = reserve_all(ctx, B->look_probes, 8 * total, B->points, 3 * n, B->normals, 3 * n, B->look_rgb, 3 * n, B->status, n)) return rc;
    CRT_HIP_CHECK(ctx, hipMemcpyAsync(B->look_probes.p, probes, (size_t)total * sizeof(crt_probe), hipMemcpyHostToDevice, stream));
    CRT_HIP_CHECK(ctx, hipMemcpyAsync(B->points.p, points, (size_t)n * 12, hipMemcpyHostToDevice, stream));
    CRT_HIP_CHECK(ctx, hipMemcpyAsync(B->normals.p, normals, (size_t)n * 12, hipMemcpyHostToDevice, stream));
    if (int rc = crt_probe_irradiance_device(ctx, volume, (const crt_probe *)B->look_probes.p, B->points.p, B->normals.p, n, B->look_rgb.p, B->status.p, stream))
        return rc;
    CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_rgb, B->look_rgb.p, (size_t)n * 12, hipMemcpyDeviceToHost, stream));
    if (out_status) CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_status, B->status.p, (size_t)n, hipMemcpyDeviceToHost, stream));
    CRT_HIP_CHECK(ctx, hipStreamSynchronize(stream));
    return CRT_OK;
}

// ---- probe-lit radiance (include/crt_hip.h: "Probe-lit radiance"; csrc/probe_lit_rule.h, csrc/kernel_probe_light.h): the DIFFUSE records of
// a radiance query take their bounce light from the volume.  The primitive enqueues probe_light_records and nothing else; the query is
// crt_query.hip's GI level loop with gi_sample_size = 0 and that launch behind every level's lighting launches (query_lit_run).

// What every probe-lit call asks, in ONE place each.  light_check: of the volume, the visibility (only when there is one) and S --
// crt_probe_irradiance_visible_device's refusals.  light_records_check: of the volume's records when there is work to do; `device`: they are
// device memory, read with 16-byte loads.
static int light_check(crt_ctx *ctx, const char *what, const crt_probe_volume *volume, const crt_probe_visibility *visibility, const uint32_t samples) {
    if (int rc = volume_check(ctx, what, volume)) return rc;
    if (visibility)
        if (int rc = visibility_check(ctx, what, visibility)) return rc;
    if (samples > 64u) return refuse(ctx, what, "gi_sample_size too large: " + std::to_string(samples) + ", at most 64");
    return CRT_OK;
}
static int light_records_check(crt_ctx *ctx, const char *what, const crt_probe_visibility *visibility, const void *probes, const void *depth, const bool device) {
    if (!probes) return refuse(ctx, what, "probes is NULL");
    if (visibility && !depth) return refuse(ctx, what, "a visibility without depth records: depth is NULL");
    if (device && ((uintptr_t)probes % 16u || (visibility && (uintptr_t)depth % 16u))) return refuse(ctx, what, "probes and depth must be aligned to 16 bytes");
    return CRT_OK;
}

int probe_light_launch(crt_ctx *ctx, const ProbeLight &L, const crt_hit *d_hits, const uint8_t *d_status, const uint64_t n, float *d_rgb, hipStream_t stream) {
    if (n == 0) return CRT_OK;
    ProbeLightArgs P{};
    P.grid = grid_of(L.volume);
    if (L.visibility) P.vis = vis_of(L.visibility);
    P.probes = (const float4 *)L.d_probes;
    P.depth = (const float2 *)L.d_depth;
    P.hits = d_hits; P.status = d_status; P.n = n; P.samples = L.samples; P.rgb = d_rgb; P.counts = L.d_counts;
    hipLaunchKernelGGL(L.visibility ? probe_light_records<true> : probe_light_records<false>, dim3(blocks_of(n)), dim3(BLOCK), 0, stream, P);
    CRT_HIP_CHECK(ctx, hipGetLastError());
    return CRT_OK;
}

extern "C" int crt_probe_light_hits_device(crt_ctx *ctx, const crt_probe_volume *volume, const crt_probe_visibility *visibility, const crt_probe *d_probes,
                                           const crt_probe_depth *d_depth, const crt_hit *d_hits, const uint8_t *d_status, uint64_t n,
                                           uint32_t gi_sample_size, float *d_rgb, uint64_t *d_counts, void *stream) {
    const char *what = "crt_probe_light_hits_device";
    if (!ctx) return CRT_ERR_INVALID;
    if (int rc = light_check(ctx, what, volume, visibility, gi_sample_size)) return rc;
    if (n == 0) return CRT_OK;
    if (n >= CRT_MAX_PIXELS) return refuse(ctx, what, "n = " + std::to_string(n) + " >= 2^31");
    if (int rc = light_records_check(ctx, what, visibility, d_probes, d_depth, true)) return rc;
    if (!d_hits || !d_status || !d_rgb) return refuse(ctx, what, "d_hits, d_status or d_rgb is NULL");
    if ((uintptr_t)d_hits % 4u || (uintptr_t)d_rgb % 4u || (uintptr_t)d_counts % 8u)
        return refuse(ctx, what, "d_hits and d_rgb must be aligned to 4 bytes, d_counts to 8");
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const ProbeLight L{volume, visibility, d_probes, visibility ? d_depth : nullptr, gi_sample_size, reinterpret_cast<unsigned long long *>(d_counts)};
    return probe_light_launch(ctx, L, d_hits, d_status, n, d_rgb, (hipStream_t)stream);
}

// the counters of the last probe-lit query, once: waits for it
static int light_harvest(crt_ctx *ctx) {
    crt_probe_state *B = ctx->probes;
    if (!B || !B->lit_open) return CRT_OK;
    CRT_HIP_CHECK(ctx, hipEventSynchronize(B->lit_ev));
    B->lit_open = false;
    B->lit_stats.lit = B->lit_pin[0];
    B->lit_stats.unlit = B->lit_pin[1];
    return CRT_OK;
}

// the start of a probe-lit query on `stream`: the refusals, before anything is enqueued; then the call's two counters, cleared
static int light_begin(crt_ctx *ctx, const char *what, const crt_ray *d_rays, const uint32_t ray_type, const crt_options *options, const float *d_rgb,
                       const crt_probe_volume *volume, const crt_probe_visibility *visibility, const crt_probe *d_probes, const crt_probe_depth *d_depth,
                       hipStream_t stream, ProbeLight *L) {
    if (int rc = query_lit_check(ctx, what, d_rays, options, d_rgb, ray_type)) return rc;
    if (int rc = light_check(ctx, what, volume, visibility, options->gi_sample_size)) return rc;
    if (int rc = light_records_check(ctx, what, visibility, d_probes, d_depth, true)) return rc;
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    CRT_HIP_CHECK(ctx, hipStreamIsCapturing(stream, &status));
    if (status != hipStreamCaptureStatusNone)
        return refuse(ctx, what, "the stream is being captured and the call waits once a recursion level (there is no enqueue-only form)");
    if (ctx->pending)
        if (int rc = crt_wait(ctx)) return rc;
    if (int rc = probes_state(ctx)) return rc;
    crt_probe_state *B = ctx->probes;
    if (int rc = B->lit_counts.reserve(ctx, 2)) return rc;
    if (!B->lit_pin) CRT_HIP_CHECK(ctx, hipHostMalloc((void **)&B->lit_pin, 2 * sizeof(unsigned long long)));
    if (!B->lit_ev) CRT_HIP_CHECK(ctx, hipEventCreate(&B->lit_ev));
    if (int rc = light_harvest(ctx)) return rc;   // the last call's counters leave the pinned words before this call's copy lands there
    B->lit_stats = crt_probe_lit_stats{};         // (a call that fails from here on leaves no other call's counts behind)
    CRT_HIP_CHECK(ctx, hipMemsetAsync(B->lit_counts.p, 0, 2 * sizeof(unsigned long long), stream));
    *L = ProbeLight{volume, visibility, d_probes, visibility ? d_depth : nullptr, options->gi_sample_size, B->lit_counts.p};
    return CRT_OK;
}

// ... and its end: the counters on their way to pinned memory, behind the call's last launch
static int light_end(crt_ctx *ctx, hipStream_t stream) {
    crt_probe_state *B = ctx->probes;
    CRT_HIP_CHECK(ctx, hipMemcpyAsync(B->lit_pin, B->lit_counts.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    CRT_HIP_CHECK(ctx, hipEventRecord(B->lit_ev, stream));
    B->lit_open = true;
    return CRT_OK;
}

extern "C" int crt_shoot_rays_lit_device(crt_ctx *ctx, const crt_ray *d_rays, uint64_t n, uint32_t ray_type, const crt_options *options,
                                         const crt_probe_volume *volume, const crt_probe_visibility *visibility, const crt_probe *d_probes,
                                         const crt_probe_depth *d_depth, float *d_rgb, void *stream) {
    const char *what = "crt_shoot_rays_lit_device";
    if (!ctx) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    ProbeLight L{};
    int rc;
    if ((rc = light_begin(ctx, what, d_rays, ray_type, options, d_rgb, volume, visibility, d_probes, d_depth, (hipStream_t)stream, &L)) ||
        (rc = query_lit_run(ctx, what, d_rays, n, ray_type, options, &L, d_rgb, (hipStream_t)stream)))
        return rc;
    return light_end(ctx, (hipStream_t)stream);
}

// the volume's records on the device for the host variants: the lookup calls' copies
static int light_upload(crt_ctx *ctx, const crt_probe_volume *volume, const crt_probe *probes, const crt_probe_depth *depth, hipStream_t stream) {
    crt_probe_state *B = ctx->probes;
    const uint64_t total = crt_probe_count(grid_of(volume));
    if (int rc = reserve_all(ctx, B->look_probes, 8 * total, B->look_depth, depth ? CRT_PROBE_DEPTH_TEXELS * total : 0)) return rc;
    CRT_HIP_CHECK(ctx, hipMemcpyAsync(B->look_probes.p, probes, (size_t)total * sizeof(crt_probe), hipMemcpyHostToDevice, stream));
    if (depth) CRT_HIP_CHECK(ctx, hipMemcpyAsync(B->look_depth.p, depth, (size_t)total * sizeof(crt_probe_depth), hipMemcpyHostToDevice, stream));
    return CRT_OK;
}

extern "C" int crt_shoot_rays_lit(crt_ctx *ctx, const crt_ray *rays, uint64_t n, uint32_t ray_type, const crt_options *options, const crt_probe_volume *volume,
                                  const crt_probe_visibility *visibility, const crt_probe *probes, const crt_probe_depth *depth, float *out_rgb) {
    const char *what = "crt_shoot_rays_lit";
    if (!ctx) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    if (int rc = query_lit_check(ctx, what, rays, options, out_rgb, ray_type)) return rc;
    if (int rc = light_check(ctx, what, volume, visibility, options->gi_sample_size)) return rc;
    if (int rc = light_records_check(ctx, what, visibility, probes, depth, false)) return rc;
    if (n >= CRT_MAX_PIXELS) return refuse(ctx, what, "n = " + std::to_string(n) + " >= 2^31");
    if (ctx->pending)
        if (int rc = crt_wait(ctx)) return rc;
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (int rc = probes_state(ctx)) return rc;
    crt_probe_state *B = ctx->probes;
    hipStream_t stream = ctx->stream;
    if (int rc = reserve_all(ctx, B->lit_rays, n, B->look_rgb, 3 * n)) return rc;
    if (int rc = light_upload(ctx, volume, probes, visibility ? depth : nullptr, stream)) return rc;
    CRT_HIP_CHECK(ctx, hipMemcpyAsync(B->lit_rays.p, rays, (size_t)n * sizeof(crt_ray), hipMemcpyHostToDevice, stream));
    if (int rc = crt_shoot_rays_lit_device(ctx, B->lit_rays.p, n, ray_type, options, volume, visibility, (const crt_probe *)B->look_probes.p,
                                           visibility ? (const crt_probe_depth *)B->look_depth.p : nullptr, B->look_rgb.p, stream))
        return rc;
    CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_rgb, B->look_rgb.p, (size_t)n * 12, hipMemcpyDeviceToHost, stream));
    CRT_HIP_CHECK(ctx, hipStreamSynchronize(stream));
    return CRT_OK;
}

// crt_render_probe_lit (`host` false: the records are device memory) and crt_render_probe_lit_host (true: host memory, uploaded first)
static int render_lit(crt_ctx *ctx, const char *what, const crt_probe_volume *volume, const crt_probe_visibility *visibility, const crt_probe *d_probes,
                      const crt_probe_depth *d_depth, const crt_options *options, float *out_rgb, uint8_t *out_rgb8, const bool host) {
    if (!ctx) return CRT_ERR_INVALID;
    const uint64_t pixels = (uint64_t)ctx->width * ctx->height;
    if (int rc = pixels_check(ctx, what, pixels)) return rc;
    if (pixels == 0) return CRT_OK;
    if (!options) return refuse(ctx, what, "options is NULL");
    if (ctx->pending)
        if (int rc = crt_wait(ctx)) return rc;
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (int rc = probes_state(ctx)) return rc;
    crt_probe_state *B = ctx->probes;
    hipStream_t stream = ctx->stream;
    if (int rc = B->lit_rays.reserve(ctx, pixels)) return rc;
    // what the query would refuse, asked before the frame under way is ended and anything is enqueued
    if (int rc = query_lit_check(ctx, what, B->lit_rays.p, options, ctx->d_frame, CRT_RAY_PRIMARY)) return rc;
    if (int rc = light_check(ctx, what, volume, visibility, options->gi_sample_size)) return rc;
    if (int rc = light_records_check(ctx, what, visibility, d_probes, d_depth, !host)) return rc;
    giframe_reset(ctx);   // the persistent colour buffer is this frame's now, as after crt_render*
    int rc;
    if (host) {
        if ((rc = light_upload(ctx, volume, d_probes, visibility ? d_depth : nullptr, stream))) return rc;
        d_probes = (const crt_probe *)B->look_probes.p;
        d_depth = visibility ? (const crt_probe_depth *)B->look_depth.p : nullptr;
    }
    if ((rc = crt_camera_rays_device(ctx, B->lit_rays.p, stream)) ||
        (rc = crt_shoot_rays_lit_device(ctx, B->lit_rays.p, pixels, CRT_RAY_PRIMARY, options, volume, visibility, d_probes, d_depth, ctx->d_frame, stream)))
        return rc;
    if (out_rgb) CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_rgb, ctx->d_frame, 3 * pixels * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (out_rgb8) {
        if ((rc = crt_quantize_device(ctx, ctx->d_frame, 3 * pixels, ctx->d_quant, stream))) return rc;
        CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_rgb8, ctx->d_quant, 3 * pixels, hipMemcpyDeviceToHost, stream));
    }
    CRT_HIP_CHECK(ctx, hipStreamSynchronize(stream));
    return CRT_OK;
}

extern "C" int crt_render_probe_lit(crt_ctx *ctx, const crt_probe_volume *volume, const crt_probe_visibility *visibility, const crt_probe *d_probes,
                                    const crt_probe_depth *d_depth, const crt_options *options, float *out_rgb, uint8_t *out_rgb8) {
    return render_lit(ctx, "crt_render_probe_lit", volume, visibility, d_probes, d_depth, options, out_rgb, out_rgb8, false);
}

extern "C" int crt_render_probe_lit_host(crt_ctx *ctx, const crt_probe_volume *volume, const crt_probe_visibility *visibility, const crt_probe *probes,
                                         const crt_probe_depth *depth, const crt_options *options, float *out_rgb, uint8_t *out_rgb8) {
    return render_lit(ctx, "crt_render_probe_lit_host", volume, visibility, probes, depth, options, out_rgb, out_rgb8, true);
}

extern "C" int crt_get_probe_lit_stats(crt_ctx *ctx, crt_probe_lit_stats *out) {
    if (!ctx || !out) return CRT_ERR_INVALID;
    *out = crt_probe_lit_stats{};
    if (!ctx->probes) return CRT_OK;
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (int rc = light_harvest(ctx)) return rc;
    *out = ctx->probes->lit_stats;
    return CRT_OK;
}

extern "C" int crt_get_probe_stats(crt_ctx *ctx, crt_probe_stats *out) {
    if (!ctx || !out) return CRT_ERR_INVALID;
    *out = ctx->probes ? ctx->probes->stats : crt_probe_stats{};
    return CRT_OK;
}
