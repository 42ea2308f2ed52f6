// crt_guides.hip -- the chain guides' own kernel (include/crt_hip.h: "Chain guides"): the layout of the caller's work area and the launch
// of guide_step for crt_guide_rays* (crt_query.hip), which owns the loop -- one trace of the live chains, then this launch, a bounce.
// Kernel: csrc/kernel_guides.h.  Everything here only enqueues: one launch, no wait, no allocation, no readback.
#include "crt_internal.h"

namespace {
#include "kernel_guides.h"
}  // namespace

static_assert(GUIDE_COUNT_WORDS > GUIDE_MAX_BOUNCES + 1u, "one count word a level");
static_assert(sizeof(crt_hit) == 48 && sizeof(crt_ray) == 24, "guide_step reads and writes the two records word by word");

// The work area: the levels' count words, the level's hit records, and two lists (level k reads list k & 1 and appends to the other):
// ray, pixel, path length, first mesh.  512 + 120 n bytes.
extern "C" size_t crt_guide_work_bytes(uint64_t n) {
    return GUIDE_COUNT_WORDS * sizeof(uint32_t) + (size_t)n * (sizeof(crt_hit) + 2 * (sizeof(crt_ray) + 3 * sizeof(uint32_t)));
}

GuideWork guides_work(void *d_work, const uint64_t n) {
    GuideWork W{};
    char *p = static_cast<char *>(d_work);
    W.count = reinterpret_cast<uint32_t *>(p); p += GUIDE_COUNT_WORDS * sizeof(uint32_t);
    W.hits = reinterpret_cast<crt_hit *>(p); p += n * sizeof(crt_hit);
    for (int k = 0; k < 2; k++) { W.rays[k] = reinterpret_cast<crt_ray *>(p); p += n * sizeof(crt_ray); }
    for (int k = 0; k < 2; k++) { W.pixel[k] = reinterpret_cast<uint32_t *>(p); p += n * sizeof(uint32_t); }
    for (int k = 0; k < 2; k++) { W.tsum[k] = reinterpret_cast<float *>(p); p += n * sizeof(float); }
    for (int k = 0; k < 2; k++) { W.mesh0[k] = reinterpret_cast<uint32_t *>(p); p += n * sizeof(uint32_t); }
    return W;
}

// level `level` <= max_bounces <= 63 of a call of 0 < n <= 2^30 rays, behind the level's trace into W.hits; level 0's rays are d_rays
int guides_launch_step(crt_ctx *ctx, const GuideWork &W, const crt_ray *d_rays, uint32_t n, uint32_t level, uint32_t max_bounces, float reflection_bias,
                       float refraction_bias, crt_hit *d_out_hits, uint8_t *d_out_status, crt_ray *d_out_last_rays, hipStream_t stream) {
    const int cur = (int)(level & 1u);
    GuideArgs G{};
    G.s = (scene_args_p)ctx->d_scene;
    G.rays = level ? W.rays[cur] : d_rays;
    G.hits = W.hits;
    if (level) { G.pixel = W.pixel[cur]; G.tsum = W.tsum[cur]; G.mesh0 = W.mesh0[cur]; G.n_dev = W.count + level; }
    G.child_rays = W.rays[cur ^ 1]; G.child_pixel = W.pixel[cur ^ 1]; G.child_tsum = W.tsum[cur ^ 1]; G.child_mesh0 = W.mesh0[cur ^ 1];
    G.child_count = W.count + level + 1;
    G.out_hits = d_out_hits; G.out_status = d_out_status; G.out_last_rays = d_out_last_rays;
    G.n = n; G.level = level; G.max_bounces = max_bounces;
    G.reflection_bias = reflection_bias; G.refraction_bias = refraction_bias;
    hipLaunchKernelGGL(guide_step, dim3((uint32_t)(((uint64_t)n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, G);
    CRT_HIP_CHECK(ctx, hipGetLastError());
    return CRT_OK;
}
