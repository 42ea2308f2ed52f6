// crt_testhooks.hip -- unit-test hooks: in libcrt_hip_test.so only (the tests load that flavour; crt_main, crt_animation and bench.py the plain one).
#include "crt_internal.h"
#include "crt_multi.h"
#include "glibc_powf.h"
#include "glibc_sincosf.h"
#include "gi_random.h"
#include "shadow_place.h"

namespace {
// unit-test kernel: the device build of csrc/glibc_powf.h
__global__ void pow5_kernel(const float *x, float *out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = crt_pow5(x[i]);
}

}  // namespace

// Unit-test hook: evaluates the device build of the restated glibc powf(x, 5) (csrc/glibc_powf.h) on host arrays.
extern "C" int crt_test_pow5(int device, const float *x, float *out, uint64_t n) {
    if (!x || !out) return CRT_ERR_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return CRT_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return CRT_ERR_HIP;
    float *dx = nullptr, *dout = nullptr;
    if (hipMalloc((void **)&dx, n * sizeof(float)) != hipSuccess) return CRT_ERR_NOMEM;
    if (hipMalloc((void **)&dout, n * sizeof(float)) != hipSuccess) { (void)hipFree(dx); return CRT_ERR_NOMEM; }
    int rc = CRT_OK;
    if (hipMemcpy(dx, x, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) rc = CRT_ERR_HIP;
    if (rc == CRT_OK && n) {
        hipLaunchKernelGGL(pow5_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, 0, dx, dout, n);
        if (hipGetLastError() != hipSuccess || hipMemcpy(out, dout, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) rc = CRT_ERR_HIP;
    }
    (void)hipFree(dx);
    (void)hipFree(dout);
    return rc;
}

__host__ __device__ static inline uint32_t gi_test_value(uint32_t what, uint32_t a, uint32_t b) {
    float f;
    memcpy(&f, &a, sizeof(f));
    float r = 0;
    switch (what) {
        case 0: r = crt_sinf(f); break;
        case 1: r = crt_cosf(f); break;
        case 2: r = crt_gi_uniform(a, b); break;
        default: return crt_gi_mix(a, b);
    }
    uint32_t u;
    memcpy(&u, &r, sizeof(u));
    return u;
}
__global__ void gi_test_kernel(uint32_t what, const uint32_t *a, const uint32_t *b, uint32_t *out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = gi_test_value(what, a[i], b ? b[i] : 0u);
}
// Unit-test hook: the GI mode's sinf / cosf / generator (csrc/glibc_sincosf.h, csrc/gi_random.h) on host arrays.
extern "C" int crt_test_gi(int device, uint32_t what, const uint32_t *a, const uint32_t *b, uint32_t *out, uint64_t n) {
    if (!a || !out || what > 3u || (what >= 2u && !b)) return CRT_ERR_INVALID;
    if (device < 0) {
        for (uint64_t i = 0; i < n; i++) out[i] = gi_test_value(what, a[i], b ? b[i] : 0u);
        return CRT_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) return CRT_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return CRT_ERR_HIP;
    uint32_t *da = nullptr, *db = nullptr, *dout = nullptr;
    int rc = CRT_OK;
    if (hipMalloc((void **)&da, (n ? n : 1) * 4) != hipSuccess || hipMalloc((void **)&db, (n ? n : 1) * 4) != hipSuccess ||
        hipMalloc((void **)&dout, (n ? n : 1) * 4) != hipSuccess) rc = CRT_ERR_NOMEM;
    if (rc == CRT_OK && n) {
        if (hipMemcpy(da, a, n * 4, hipMemcpyHostToDevice) != hipSuccess || (b && hipMemcpy(db, b, n * 4, hipMemcpyHostToDevice) != hipSuccess)) rc = CRT_ERR_HIP;
        if (rc == CRT_OK) {
            hipLaunchKernelGGL(gi_test_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, 0, what, da, b ? db : nullptr, dout, n);
            if (hipGetLastError() != hipSuccess || hipMemcpy(out, dout, n * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = CRT_ERR_HIP;
        }
    }
    if (da) (void)hipFree(da);
    if (db) (void)hipFree(db);
    if (dout) (void)hipFree(dout);
    return rc;
}

extern "C" int crt_debug_multi_force_staged(crt_multi *M, int on) {
    if (!M) return CRT_ERR_INVALID;
    M->force_staged = on != 0;
    M->cached_rects.clear();  // the next render allocates the pinned buffers
    return CRT_OK;
}

extern "C" int crt_debug_multi_fail_next_alloc(crt_multi *M) {
    if (!M) return CRT_ERR_INVALID;
    M->fail_next_alloc = true;
    return CRT_OK;
}

// Unit-test hook: lowers the number of stack entries the filter walks may use (SceneArgs::bvh_stack) on a live context -- at least 1,
// never above what crt_create sized the spill regions for (a larger value restores it) -- so that the walks' "stack too small" exits
// run: kernel_bvh.h, give_up.  Waits for everything the context has enqueued, then uploads the scene's argument block again.
extern "C" int crt_debug_set_filter_stack(crt_ctx *ctx, uint32_t entries) {
    if (!ctx) return CRT_ERR_INVALID;
    if (!ctx->scene.bvh_ok || !ctx->bvh_stack_built) { ctx->error = "the scene has no filter"; return CRT_ERR_INVALID; }
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    CRT_HIP_CHECK(ctx, hipDeviceSynchronize());
    ctx->scene.bvh_stack = entries < 1u ? 1u : (entries > ctx->bvh_stack_built ? ctx->bvh_stack_built : entries);
    CRT_HIP_CHECK(ctx, hipMemcpy(ctx->d_scene, &ctx->scene, sizeof(SceneArgs), hipMemcpyHostToDevice));
    return CRT_OK;
}

// Unit-test hook: the queries' chunk sizes (crt_ctx::query_host_rays, query_launch_rays, shoot_pass_rays) on a live context, so that a
// few thousand rays run crt_query.hip's chunk loops.  0 restores a default; other values are clamped to [64, the default].  Waits for
// everything the context has enqueued.
extern "C" int crt_debug_set_query_chunks(crt_ctx *ctx, uint64_t host_rays, uint64_t launch_rays, uint64_t pass_rays) {
    if (!ctx) return CRT_ERR_INVALID;
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    CRT_HIP_CHECK(ctx, hipDeviceSynchronize());
    const auto chunk = [](uint64_t v, uint64_t dflt) { return v == 0 ? dflt : std::min(std::max<uint64_t>(v, 64u), dflt); };
    ctx->query_host_rays = chunk(host_rays, QUERY_HOST_RAYS);
    ctx->query_launch_rays = chunk(launch_rays, QUERY_LAUNCH_RAYS);
    ctx->shoot_pass_rays = chunk(pass_rays, SHOOT_PASS_RAYS);
    return CRT_OK;
}

// Unit-test hook: crt_bake_probes takes `probes` probes per chunk from now on (0: as many as fit its scratch again)
extern "C" int crt_debug_set_probe_chunk(crt_ctx *ctx, uint32_t probes) {
    if (!ctx) return CRT_ERR_INVALID;
    ctx->probe_chunk = std::min<uint32_t>(probes, 1u << 24);
    return CRT_OK;
}

// Unit-test hook: level 0's fixed shadow slots (csrc/shadow_place.h) -- every slot of items x samples work items and n_lights lights through the
// inverse placement and back through the forward one, on the host; *mismatches = the slots that do not come back.
extern "C" int crt_test_shadow_place(uint32_t items, uint32_t samples, uint32_t n_lights, uint64_t *mismatches) {
    if (!mismatches || !items || !samples || !n_lights || (uint64_t)items * samples * 64u * n_lights >= (1ull << 31)) return CRT_ERR_INVALID;
    *mismatches = level0_slot_mismatches(items * samples, n_lights);
    return CRT_OK;
}
