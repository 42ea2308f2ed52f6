#include "RayTracer.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <thread>

namespace crt {

std::vector<crt_rect> bucketRectangles(unsigned int width, unsigned int height, unsigned int bucketSize,
                                       RenderOptimization optimization, unsigned int hardwareConcurrency) {
  // RayTracer::render's switch (RayTracer.cpp:209-286); both counters are `unsigned short` members
  // (RayTracer.h:74-75), so the values wrap at 65536 like the reference's do.
  unsigned short threadCount = 1, rectangleCount = 1;
  bool regions = true;
  switch (optimization) {
    case NoOptimization: case AABB: case BVH:
      break;
    case Regions:
      threadCount = (unsigned short)hardwareConcurrency;
      rectangleCount = (unsigned short)hardwareConcurrency;
      break;
    default:  // the six bucket modes
      threadCount = (unsigned short)hardwareConcurrency;
      rectangleCount = (unsigned short)bucketSize;
      regions = false;
      break;
  }
  std::vector<crt_rect> rects;
  unsigned int threadNumY = static_cast<unsigned int>(std::sqrt(rectangleCount));  // RayTracer.cpp:115,143
  if (threadNumY == 0) threadNumY = 1;
  unsigned int threadNumX = rectangleCount / threadNumY;
  if (threadNumX == 0 || width == 0 || height == 0) return rects;  // the reference divides by zero here
  unsigned int regionWidth = width / threadNumX;
  unsigned int regionHeight = height / threadNumY;
  if (regions && threadCount == 1) {  // RayTracer.cpp:123-126
    rects.push_back(crt_rect{0, 0, regionWidth, regionHeight});
    return rects;
  }
  const int count = regions ? threadCount : rectangleCount;  // RayTracer.cpp:130 vs :149
  for (int i = 0; i < count; i++) {
    unsigned column = (i * regionWidth) % width;
    unsigned row = (i / threadNumX) * regionHeight;
    rects.push_back(crt_rect{row, column, regionWidth, regionHeight});
  }
  return rects;
}

// ------------------------------------------------------------------------------------------------ PPM
namespace {
struct DecimalTable {
  char text[256][4];
  unsigned char len[256];
  DecimalTable() {
    for (int i = 0; i < 256; i++) len[i] = (unsigned char)snprintf(text[i], 4, "%d", i);
  }
};
const DecimalTable &decimals() {
  static const DecimalTable t;
  return t;
}
inline unsigned short quantise(float c) {  // PPMColor, Color.cpp:12-16: clamp, scale, TRUNCATE
  const float cl = (c < 0.0f) ? 0.0f : ((1.0f < c) ? 1.0f : c);
  return static_cast<unsigned short>(cl * 255);
}
template <typename Fetch>
void writePPMImpl(const std::string &path, unsigned int width, unsigned int height, Fetch fetch) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f) throw std::runtime_error("cannot open " + path + " for writing");
  // RayTracer.cpp:541-551: "P3\n{W} {H}\n255\n", then per row "{r} {g} {b}\t" per pixel and "\n"
  fprintf(f, "P3\n%u %u\n%d\n", width, height, 255);
  const DecimalTable &t = decimals();
  std::vector<char> line((size_t)width * 12 + 2);
  for (unsigned int row = 0; row < height; row++) {
    char *p = line.data();
    for (unsigned int col = 0; col < width; col++) {
      for (int k = 0; k < 3; k++) {
        const unsigned v = fetch(((size_t)row * width + col) * 3 + k);
        memcpy(p, t.text[v], t.len[v]);
        p += t.len[v];
        *p++ = (k == 2) ? '\t' : ' ';
      }
    }
    *p++ = '\n';
    fwrite(line.data(), 1, (size_t)(p - line.data()), f);
  }
  fclose(f);
}
}  // namespace

void writePPM(const std::string &path, const float *rgb, unsigned int width, unsigned int height) {
  writePPMImpl(path, width, height, [rgb](size_t i) -> unsigned { return quantise(rgb[i]); });
}

void writePPMQuantized(const std::string &path, const uint8_t *rgb8, unsigned int width, unsigned int height) {
  writePPMImpl(path, width, height, [rgb8](size_t i) -> unsigned { return rgb8[i]; });
}

// ------------------------------------------------------------------------------------------------ RayTracer
RayTracer::RayTracer(Scene &scene, int device, const crt_tuning *tuning)
    : accelerationStructure(scene), scene(scene), camera(scene.camera) {
  flattenScene(scene, accelerationStructure, flat);
  int rc = crt_create_tuned(&flat.desc, device, tuning, &ctx);
  if (rc != CRT_OK) throw std::runtime_error(std::string("crt_create failed: ") + crt_last_error(nullptr));
  deviceIndex = device;
  if (tuning) { tuningCopy = *tuning; haveTuning = true; }
  {  // the context starts with the scene's camera, as RayTracer::RayTracer copies scene.camera (RayTracer.cpp:46)
    const float pos[3] = {camera.getPosition().x, camera.getPosition().y, camera.getPosition().z};
    crt_set_camera(ctx, pos, &camera.getRotationMatrix().m[0][0]);
  }
  frame.assign((size_t)scene.sceneSettings.image.width * scene.sceneSettings.image.height * 3, 0.0f);
}

RayTracer::RayTracer(Scene &scene, const std::vector<int> &devices, const crt_tuning *tuning)
    : accelerationStructure(scene), scene(scene), camera(scene.camera) {
  flattenScene(scene, accelerationStructure, flat);
  int rc = crt_multi_create(&flat.desc, devices.data(), (uint32_t)devices.size(), tuning, &multi);
  if (rc != CRT_OK) throw std::runtime_error(std::string("crt_multi_create failed: ") + crt_multi_last_error(nullptr));
  const float pos[3] = {camera.getPosition().x, camera.getPosition().y, camera.getPosition().z};
  crt_multi_set_camera(multi, pos, &camera.getRotationMatrix().m[0][0]);
  frame.assign((size_t)scene.sceneSettings.image.width * scene.sceneSettings.image.height * 3, 0.0f);
}

RayTracer::~RayTracer() {
  for (size_t i = 0; i < ring.size(); i++) {
    if (ring[i].busy) crt_wait(ring[i].ctx);
    crt_free_pinned(ring[i].rgb8);
    if (i > 0) crt_destroy(ring[i].ctx);
  }
  crt_destroy(ctx);
  crt_multi_destroy(multi);
}

void RayTracer::setFramesInFlight(unsigned int k) {
  if (multi) throw std::runtime_error("frames in flight: not available on a multi-device tracer");
  if (k < 1) k = 1;
  if (k > 8) k = 8;
  const size_t bytes = (size_t)scene.sceneSettings.image.width * scene.sceneSettings.image.height * 3;
  while (ring.size() < k) {
    InFlight f;
    if (ring.empty()) f.ctx = ctx;
    else if (crt_create_tuned(&flat.desc, deviceIndex, haveTuning ? &tuningCopy : nullptr, &f.ctx) != CRT_OK)
      throw std::runtime_error(std::string("crt_create failed: ") + crt_last_error(nullptr));
    f.rgb8 = static_cast<uint8_t *>(crt_alloc_pinned(bytes));
    if (!f.rgb8) { if (!ring.empty()) crt_destroy(f.ctx); throw std::runtime_error("out of pinned host memory"); }
    ring.push_back(f);
  }
}

int RayTracer::renderAsync(const RenderOptions &ro) {
  if (ring.empty()) setFramesInFlight(2);
  const int slot = (int)(ringNext % ring.size());
  ringNext++;
  InFlight &f = ring[(size_t)slot];
  if (f.busy) { crt_wait(f.ctx); f.busy = false; }  // the slot's previous frame (its pixels are overwritten from here on)
  crt_options o{};
  o.max_depth = ro.MAX_DEPTH;
  o.shadow_bias = ro.SHADOW_BIAS;
  o.reflection_bias = ro.REFLECTION_BIAS;
  o.refraction_bias = ro.REFRACTION_BIAS;
  o.use_gi = ro.USE_GI ? 1u : 0u;
  o.gi_sample_size = ro.GI_SAMPLE_SIZE;
  o.rays_per_pixel = ro.RAYS_PER_PIXEL;
  o.monte_carlo_bias = ro.MONTE_CARLO_BIAS;
  o.gi_seed = ro.USE_GI ? giSeed++ : 0u;  // every GI frame its own seed, as every GI render of the reference differs
  const Matrix3 &m = camera.getRotationMatrix();
  const float pos[3] = {camera.getPosition().x, camera.getPosition().y, camera.getPosition().z};
  int rc = crt_set_camera(f.ctx, pos, &m.m[0][0]);
  const unsigned int W = scene.sceneSettings.image.width, H = scene.sceneSettings.image.height;
  std::vector<crt_rect> rects = bucketRectangles(W, H, scene.sceneSettings.bucketSize, ro.optimization, std::thread::hardware_concurrency());
  if (rc == CRT_OK) rc = crt_render_async(f.ctx, &o, rects.data(), (uint32_t)rects.size(), nullptr, f.rgb8);
  if (rc != CRT_OK) throw std::runtime_error(std::string("renderAsync failed: ") + crt_last_error(f.ctx));
  f.busy = true;
  return slot;
}

const uint8_t *RayTracer::finishFrame(int slot) {
  if (slot < 0 || (size_t)slot >= ring.size()) throw std::runtime_error("finishFrame: no such slot");
  InFlight &f = ring[(size_t)slot];
  if (f.busy) {
    if (crt_wait(f.ctx) != CRT_OK) throw std::runtime_error(std::string("finishFrame failed: ") + crt_last_error(f.ctx));
    f.busy = false;
  }
  return f.rgb8;
}

// ------------------------------------------------------------------------------------------------ ray queries
std::vector<crt_hit> RayTracer::traceRays(const std::vector<crt_ray> &rays, unsigned int rayType) {
  if (multi) throw std::runtime_error("traceRays: not available on a multi-device tracer");
  std::vector<crt_hit> hits(rays.size());
  if (crt_trace_rays(ctx, rays.data(), rays.size(), rayType, hits.data()) != CRT_OK)
    throw std::runtime_error(std::string("traceRays failed: ") + crt_last_error(ctx));
  return hits;
}

std::vector<crt_hit> RayTracer::guideRays(const std::vector<crt_ray> &rays, const RenderOptions &renderOptions, unsigned int maxBounces, unsigned int rayType,
                                          std::vector<unsigned char> *status, std::vector<crt_ray> *lastRays) {
  if (multi) throw std::runtime_error("guideRays: not available on a multi-device tracer");
  std::vector<crt_hit> hits(rays.size());
  if (status) status->assign(rays.size(), 0);
  if (lastRays) lastRays->assign(rays.size(), crt_ray{});
  crt_options options{};
  options.reflection_bias = renderOptions.REFLECTION_BIAS;
  options.refraction_bias = renderOptions.REFRACTION_BIAS;
  if (crt_guide_rays(ctx, rays.data(), rays.size(), rayType, &options, maxBounces, hits.data(), status ? status->data() : nullptr,
                     lastRays ? lastRays->data() : nullptr) != CRT_OK)
    throw std::runtime_error(std::string("guideRays failed: ") + crt_last_error(ctx));
  return hits;
}

void RayTracer::setGuideBounces(unsigned int maxBounces) {
  if (multi) throw std::runtime_error("setGuideBounces: not available on a multi-device tracer");
  if (crt_set_guide_bounces(ctx, maxBounces) != CRT_OK) throw std::runtime_error(std::string("setGuideBounces failed: ") + crt_last_error(ctx));
}

void RayTracer::setVarianceEstimate(const crt_variance_estimate *estimate) {
  if (multi) throw std::runtime_error("setVarianceEstimate: not available on a multi-device tracer");
  if (crt_set_variance_estimate(ctx, estimate) != CRT_OK) throw std::runtime_error(std::string("setVarianceEstimate failed: ") + crt_last_error(ctx));
}

unsigned int RayTracer::guideBounces() const { return multi ? 0u : crt_guide_bounces(ctx); }

std::vector<unsigned char> RayTracer::occludedRays(const std::vector<crt_ray> &rays, const std::vector<float> &maxDistance) {
  if (multi) throw std::runtime_error("occludedRays: not available on a multi-device tracer");
  if (maxDistance.size() != rays.size()) throw std::runtime_error("occludedRays: one max distance per ray");
  std::vector<unsigned char> out(rays.size());
  if (crt_occluded_rays(ctx, rays.data(), maxDistance.data(), rays.size(), out.data()) != CRT_OK)
    throw std::runtime_error(std::string("occludedRays failed: ") + crt_last_error(ctx));
  return out;
}

std::vector<crt_ray> RayTracer::cameraRays() {
  if (multi) throw std::runtime_error("cameraRays: not available on a multi-device tracer");
  const size_t n = (size_t)scene.sceneSettings.image.width * scene.sceneSettings.image.height;
  const Matrix3 &m = camera.getRotationMatrix();
  const float pos[3] = {camera.getPosition().x, camera.getPosition().y, camera.getPosition().z};
  // page-locked host memory is the device's to write: the rays need no device buffer of this layer's own
  crt_ray *pinned = static_cast<crt_ray *>(crt_alloc_pinned((n ? n : 1) * sizeof(crt_ray)));
  if (!pinned) throw std::runtime_error("out of pinned host memory");
  int rc = crt_set_camera(ctx, pos, &m.m[0][0]);
  if (rc == CRT_OK) rc = crt_camera_rays_device(ctx, pinned, nullptr);
  if (rc == CRT_OK) rc = crt_synchronize(ctx);
  std::vector<crt_ray> rays;
  if (rc == CRT_OK) rays.assign(pinned, pinned + n);
  crt_free_pinned(pinned);
  if (rc != CRT_OK) throw std::runtime_error(std::string("cameraRays failed: ") + crt_last_error(ctx));
  return rays;
}

std::vector<float> RayTracer::shadeHits(const std::vector<crt_hit> &hits, float shadowBias, std::vector<unsigned char> *status) {
  if (multi) throw std::runtime_error("shadeHits: not available on a multi-device tracer");
  std::vector<float> rgb(hits.size() * 3);
  if (status) status->assign(hits.size(), 0);
  crt_options options{};
  options.shadow_bias = shadowBias;
  if (crt_shade_hits(ctx, hits.data(), hits.size(), &options, rgb.data(), status ? status->data() : nullptr) != CRT_OK)
    throw std::runtime_error(std::string("shadeHits failed: ") + crt_last_error(ctx));
  return rgb;
}

std::vector<float> RayTracer::lightPoints(const std::vector<float> &points, const std::vector<float> &normals, float shadowBias) {
  if (multi) throw std::runtime_error("lightPoints: not available on a multi-device tracer");
  if (points.size() % 3 || normals.size() != points.size()) throw std::runtime_error("lightPoints: three floats per point, one normal per point");
  std::vector<float> out(points.size() / 3);
  if (crt_light_points(ctx, points.data(), normals.data(), out.size(), shadowBias, out.data()) != CRT_OK)
    throw std::runtime_error(std::string("lightPoints failed: ") + crt_last_error(ctx));
  return out;
}

std::vector<float> RayTracer::shootRays(const std::vector<crt_ray> &rays, const RenderOptions &ro, unsigned int rayType, crt_shoot_stats *stats) {
  if (multi) throw std::runtime_error("shootRays: not available on a multi-device tracer");
  std::vector<float> rgb(rays.size() * 3);
  crt_options options{};
  options.max_depth = ro.MAX_DEPTH;
  options.shadow_bias = ro.SHADOW_BIAS;
  options.reflection_bias = ro.REFLECTION_BIAS;
  options.refraction_bias = ro.REFRACTION_BIAS;
  options.use_gi = ro.USE_GI ? 1u : 0u;
  if (crt_shoot_rays(ctx, rays.data(), rays.size(), rayType, &options, rgb.data()) != CRT_OK)
    throw std::runtime_error(std::string("shootRays failed: ") + crt_last_error(ctx));
  if (stats && crt_get_shoot_stats(ctx, stats) != CRT_OK) throw std::runtime_error(std::string("shootRays failed: ") + crt_last_error(ctx));
  return rgb;
}

std::vector<float> RayTracer::shootRaysGI(const std::vector<crt_ray> &rays, const std::vector<uint32_t> &keys, const RenderOptions &ro, unsigned int rayType,
                                          crt_shoot_stats *stats) {
  if (multi) throw std::runtime_error("shootRaysGI: not available on a multi-device tracer");
  if (!keys.empty() && keys.size() != rays.size()) throw std::runtime_error("shootRaysGI: one key per ray, or none");
  std::vector<float> rgb(rays.size() * 3);
  crt_options options{};
  options.max_depth = ro.MAX_DEPTH;
  options.shadow_bias = ro.SHADOW_BIAS;
  options.reflection_bias = ro.REFLECTION_BIAS;
  options.refraction_bias = ro.REFRACTION_BIAS;
  options.use_gi = ro.USE_GI ? 1u : 0u;
  options.gi_sample_size = ro.GI_SAMPLE_SIZE;
  options.monte_carlo_bias = ro.MONTE_CARLO_BIAS;
  options.gi_seed = giSeed;
  if (crt_shoot_rays_gi(ctx, rays.data(), keys.empty() ? nullptr : keys.data(), rays.size(), rayType, &options, rgb.data()) != CRT_OK)
    throw std::runtime_error(std::string("shootRaysGI failed: ") + crt_last_error(ctx));
  if (stats && crt_get_shoot_stats(ctx, stats) != CRT_OK) throw std::runtime_error(std::string("shootRaysGI failed: ") + crt_last_error(ctx));
  return rgb;
}

std::vector<float> RayTracer::bakeLightmap(const std::string &pathToImage, const crt_bake &bake, const RenderOptions &ro, std::vector<unsigned char> *status,
                                           crt_bake_stats *stats) {
  if (multi) throw std::runtime_error("bakeLightmap: not available on a multi-device tracer");
  const size_t n = (size_t)bake.width * bake.height;
  std::vector<float> rgb(n * 3);
  std::vector<uint8_t> q(pathToImage.empty() ? 0 : n * 3);
  if (status) status->assign(n, 0);
  crt_options options{};
  options.max_depth = ro.MAX_DEPTH;
  options.shadow_bias = ro.SHADOW_BIAS;
  options.reflection_bias = ro.REFLECTION_BIAS;
  options.refraction_bias = ro.REFRACTION_BIAS;
  options.use_gi = ro.USE_GI ? 1u : 0u;
  options.gi_sample_size = ro.GI_SAMPLE_SIZE;
  options.monte_carlo_bias = ro.MONTE_CARLO_BIAS;
  options.gi_seed = giSeed;
  if (crt_bake_lightmap(ctx, &bake, &options, n ? rgb.data() : nullptr, q.empty() ? nullptr : q.data(), status && n ? status->data() : nullptr, nullptr) != CRT_OK)
    throw std::runtime_error(std::string("bakeLightmap failed: ") + crt_last_error(ctx));
  if (stats && crt_get_bake_stats(ctx, stats) != CRT_OK) throw std::runtime_error(std::string("bakeLightmap failed: ") + crt_last_error(ctx));
  if (!pathToImage.empty()) writePPMQuantized(pathToImage, q.data(), bake.width, bake.height);
  return rgb;
}

std::vector<crt_probe> RayTracer::bakeProbes(const crt_probe_volume &volume, const RenderOptions &ro, crt_probe_stats *stats) {
  if (multi) throw std::runtime_error("bakeProbes: not available on a multi-device tracer");
  std::vector<crt_probe> probes((size_t)volume.nx * volume.ny * volume.nz);
  crt_options options{};
  options.max_depth = ro.MAX_DEPTH;
  options.shadow_bias = ro.SHADOW_BIAS;
  options.reflection_bias = ro.REFLECTION_BIAS;
  options.refraction_bias = ro.REFRACTION_BIAS;
  options.use_gi = ro.USE_GI ? 1u : 0u;
  options.gi_sample_size = ro.GI_SAMPLE_SIZE;
  options.monte_carlo_bias = ro.MONTE_CARLO_BIAS;
  options.gi_seed = giSeed;
  if (crt_bake_probes(ctx, &volume, &options, probes.empty() ? nullptr : probes.data(), nullptr) != CRT_OK)
    throw std::runtime_error(std::string("bakeProbes failed: ") + crt_last_error(ctx));
  if (stats && crt_get_probe_stats(ctx, stats) != CRT_OK) throw std::runtime_error(std::string("bakeProbes failed: ") + crt_last_error(ctx));
  return probes;
}

std::vector<float> RayTracer::probeIrradiance(const crt_probe_volume &volume, const std::vector<crt_probe> &probes, const std::vector<float> &points,
                                              const std::vector<float> &normals, std::vector<unsigned char> *status) {
  if (multi) throw std::runtime_error("probeIrradiance: not available on a multi-device tracer");
  if (points.size() % 3 || normals.size() != points.size()) throw std::runtime_error("probeIrradiance: three floats per point, one normal per point");
  if (probes.size() != (size_t)volume.nx * volume.ny * volume.nz) throw std::runtime_error("probeIrradiance: one record per probe of the volume");
  const size_t n = points.size() / 3;
  std::vector<float> rgb(points.size());
  if (status) status->assign(n, 0);
  if (crt_probe_irradiance(ctx, &volume, probes.data(), points.data(), normals.data(), n, rgb.data(), status && n ? status->data() : nullptr) != CRT_OK)
    throw std::runtime_error(std::string("probeIrradiance failed: ") + crt_last_error(ctx));
  return rgb;
}

std::vector<crt_probe> RayTracer::bakeProbesVisible(const crt_probe_volume &volume, const crt_probe_visibility &visibility, const RenderOptions &ro,
                                                    std::vector<crt_probe_depth> *depth, crt_probe_stats *stats) {
  if (multi) throw std::runtime_error("bakeProbesVisible: not available on a multi-device tracer");
  std::vector<crt_probe> probes((size_t)volume.nx * volume.ny * volume.nz);
  if (depth) depth->assign(probes.size(), crt_probe_depth{});
  crt_options options{};
  options.max_depth = ro.MAX_DEPTH;
  options.shadow_bias = ro.SHADOW_BIAS;
  options.reflection_bias = ro.REFLECTION_BIAS;
  options.refraction_bias = ro.REFRACTION_BIAS;
  options.use_gi = ro.USE_GI ? 1u : 0u;
  options.gi_sample_size = ro.GI_SAMPLE_SIZE;
  options.monte_carlo_bias = ro.MONTE_CARLO_BIAS;
  options.gi_seed = giSeed;
  if (crt_bake_probes_visible(ctx, &volume, &visibility, &options, probes.empty() ? nullptr : probes.data(), nullptr,
                              depth && !depth->empty() ? depth->data() : nullptr, nullptr) != CRT_OK)
    throw std::runtime_error(std::string("bakeProbesVisible failed: ") + crt_last_error(ctx));
  if (stats && crt_get_probe_stats(ctx, stats) != CRT_OK) throw std::runtime_error(std::string("bakeProbesVisible failed: ") + crt_last_error(ctx));
  return probes;
}

std::vector<float> RayTracer::probeIrradianceVisible(const crt_probe_volume &volume, const crt_probe_visibility &visibility, const std::vector<crt_probe> &probes,
                                                     const std::vector<crt_probe_depth> &depth, const std::vector<float> &points,
                                                     const std::vector<float> &normals, std::vector<unsigned char> *status) {
  if (multi) throw std::runtime_error("probeIrradianceVisible: not available on a multi-device tracer");
  if (points.size() % 3 || normals.size() != points.size()) throw std::runtime_error("probeIrradianceVisible: three floats per point, one normal per point");
  if (probes.size() != (size_t)volume.nx * volume.ny * volume.nz || depth.size() != probes.size())
    throw std::runtime_error("probeIrradianceVisible: one record and one depth record per probe of the volume");
  const size_t n = points.size() / 3;
  std::vector<float> rgb(points.size());
  if (status) status->assign(n, 0);
  if (crt_probe_irradiance_visible(ctx, &volume, &visibility, probes.data(), depth.data(), points.data(), normals.data(), n, rgb.data(),
                                   status && n ? status->data() : nullptr) != CRT_OK)
    throw std::runtime_error(std::string("probeIrradianceVisible failed: ") + crt_last_error(ctx));
  return rgb;
}

std::vector<float> RayTracer::probeIrradianceView(const std::string &pathToImage, const crt_probe_volume &volume, const std::vector<crt_probe> &probes,
                                                  const crt_probe_visibility *visibility, const std::vector<crt_probe_depth> *depth) {
  const unsigned int W = scene.sceneSettings.image.width, H = scene.sceneSettings.image.height;
  const size_t n = (size_t)W * H;
  const std::vector<crt_hit> hits = traceRays(cameraRays(), CRT_RAY_PRIMARY);
  std::vector<float> points(3 * n), normals(3 * n);
  for (size_t i = 0; i < n; i++)
    for (int k = 0; k < 3; k++) { points[3 * i + k] = hits[i].point[k]; normals[3 * i + k] = hits[i].normal[k]; }
  std::vector<unsigned char> status;
  std::vector<float> rgb = visibility && depth ? probeIrradianceVisible(volume, *visibility, probes, *depth, points, normals, &status)
                                               : probeIrradiance(volume, probes, points, normals, &status);
  const Color &bg = scene.sceneSettings.sceneBackgroundColor;
  for (size_t i = 0; i < n; i++)
    if (!hits[i].hit || !status[i]) { rgb[3 * i] = bg.x; rgb[3 * i + 1] = bg.y; rgb[3 * i + 2] = bg.z; }
  if (!pathToImage.empty()) {
    // page-locked host memory is the device's to read and write: the quantisation is crt_quantize_device's
    float *in = static_cast<float *>(crt_alloc_pinned((n ? n : 1) * 3 * sizeof(float)));
    uint8_t *q = static_cast<uint8_t *>(crt_alloc_pinned((n ? n : 1) * 3));
    int rc = in && q ? CRT_OK : CRT_ERR_NOMEM;
    if (rc == CRT_OK) {
      std::copy(rgb.begin(), rgb.end(), in);
      rc = crt_quantize_device(ctx, in, 3 * n, q, nullptr);
    }
    if (rc == CRT_OK) rc = crt_synchronize(ctx);
    if (rc == CRT_OK) writePPMQuantized(pathToImage, q, W, H);
    if (in) crt_free_pinned(in);
    if (q) crt_free_pinned(q);
    if (rc != CRT_OK) throw std::runtime_error(std::string("probeIrradianceView failed: ") + (rc == CRT_ERR_NOMEM ? "out of pinned host memory" : crt_last_error(ctx)));
  }
  return rgb;
}

// renderOptions as the probe-lit calls take them: USE_GI set, GI_SAMPLE_SIZE the rule's S
static crt_options litOptions(const RenderOptions &ro, uint32_t giSeed) {
  crt_options options{};
  options.max_depth = ro.MAX_DEPTH;
  options.shadow_bias = ro.SHADOW_BIAS;
  options.reflection_bias = ro.REFLECTION_BIAS;
  options.refraction_bias = ro.REFRACTION_BIAS;
  options.use_gi = 1u;
  options.gi_sample_size = ro.GI_SAMPLE_SIZE;
  options.monte_carlo_bias = ro.MONTE_CARLO_BIAS;
  options.gi_seed = giSeed;
  return options;
}

std::vector<float> RayTracer::shootRaysLit(const std::vector<crt_ray> &rays, unsigned rayType, const RenderOptions &ro, const crt_probe_volume &volume,
                                           const std::vector<crt_probe> &probes, const crt_probe_visibility *visibility,
                                           const std::vector<crt_probe_depth> *depth) {
  if (multi) throw std::runtime_error("shootRaysLit: not available on a multi-device tracer");
  if (probes.size() != (size_t)volume.nx * volume.ny * volume.nz || (visibility && (!depth || depth->size() != probes.size())))
    throw std::runtime_error("shootRaysLit: one record per probe of the volume, and with a visibility one depth record");
  std::vector<float> rgb(3 * rays.size());
  const crt_options options = litOptions(ro, giSeed);
  if (crt_shoot_rays_lit(ctx, rays.data(), rays.size(), rayType, &options, &volume, visibility, probes.data(), visibility ? depth->data() : nullptr,
                         rgb.data()) != CRT_OK)
    throw std::runtime_error(std::string("shootRaysLit failed: ") + crt_last_error(ctx));
  return rgb;
}

std::vector<float> RayTracer::renderProbeLit(const std::string &pathToImage, const RenderOptions &ro, const crt_probe_volume &volume,
                                             const std::vector<crt_probe> &probes, const crt_probe_visibility *visibility,
                                             const std::vector<crt_probe_depth> *depth, crt_probe_lit_stats *stats) {
  if (multi) throw std::runtime_error("renderProbeLit: not available on a multi-device tracer");
  if (probes.empty() || probes.size() != (size_t)volume.nx * volume.ny * volume.nz || (visibility && (!depth || depth->size() != probes.size())))
    throw std::runtime_error("renderProbeLit: one record per probe of the volume, and with a visibility one depth record");
  const unsigned int W = scene.sceneSettings.image.width, H = scene.sceneSettings.image.height;
  const size_t n = (size_t)W * H;
  std::vector<float> rgb(3 * n);
  std::vector<uint8_t> q(3 * n);
  const crt_options options = litOptions(ro, giSeed);
  if (crt_render_probe_lit_host(ctx, &volume, visibility, probes.data(), visibility ? depth->data() : nullptr, &options, rgb.data(), q.data()) != CRT_OK ||
      (stats && crt_get_probe_lit_stats(ctx, stats) != CRT_OK))
    throw std::runtime_error(std::string("renderProbeLit failed: ") + crt_last_error(ctx));
  if (!pathToImage.empty()) writePPMQuantized(pathToImage, q.data(), W, H);
  return rgb;
}

crt_query_stats RayTracer::queryStats() const {
  crt_query_stats s{};
  if (!multi) crt_get_query_stats(ctx, &s);
  return s;
}

crt_stats RayTracer::stats() const {
  crt_stats s{};
  if (multi) crt_multi_get_stats(multi, &s);
  else crt_get_stats(ctx, &s);
  return s;
}

int RayTracer::renderFlat(const std::string &pathToImage, const RenderOptions &ro, float *outRGB, unsigned int counters) {
  const unsigned int W = scene.sceneSettings.image.width, H = scene.sceneSettings.image.height;
  crt_options o{};
  o.max_depth = ro.MAX_DEPTH;
  o.shadow_bias = ro.SHADOW_BIAS;
  o.reflection_bias = ro.REFLECTION_BIAS;
  o.refraction_bias = ro.REFRACTION_BIAS;
  o.use_gi = ro.USE_GI ? 1u : 0u;
  o.gi_sample_size = ro.GI_SAMPLE_SIZE;
  o.rays_per_pixel = ro.RAYS_PER_PIXEL;
  o.monte_carlo_bias = ro.MONTE_CARLO_BIAS;
  o.gi_seed = ro.USE_GI ? giSeed++ : 0u;  // every GI frame its own seed, as every GI render of the reference differs
  o.collect_counters = counters;  // 0, 1 (counting build) or 2 (production kernels with tallies), see crt_hip.h
  const Matrix3 &m = camera.getRotationMatrix();
  const float pos[3] = {camera.getPosition().x, camera.getPosition().y, camera.getPosition().z};
  int rc = multi ? crt_multi_set_camera(multi, pos, &m.m[0][0]) : crt_set_camera(ctx, pos, &m.m[0][0]);
  if (rc) return rc;
  // All ten modes render with the tree's semantics: the three BVH* modes are pixel-identical in the
  // reference, the non-tree modes differ from them in a handful of pixels and are not
  // part of this path.  The mode still selects the pixel coverage.
  note = ro.optimization < BVH ? "RenderOptimization " + std::to_string((int)ro.optimization) + " is rendered with the tree modes' semantics (the reference's brute-force and "
                                 "single-box modes differ from its tree modes in a handful of pixels); the mode selects the pixel coverage only" : std::string();
  std::vector<crt_rect> rects = bucketRectangles(W, H, scene.sceneSettings.bucketSize, ro.optimization,
                                                 std::thread::hardware_concurrency());
  rc = multi ? crt_multi_render(multi, &o, rects.data(), (uint32_t)rects.size(), outRGB)
             : crt_render(ctx, &o, rects.data(), (uint32_t)rects.size(), outRGB);
  if (rc) return rc;
  if (!pathToImage.empty()) {  // RayTracer.cpp:294-296; quantised on the device with the same rule
    std::vector<uint8_t> q((size_t)W * H * 3);
    rc = multi ? crt_multi_read_quantized(multi, q.data()) : crt_read_quantized(ctx, q.data());
    if (rc) return rc;
    writePPMQuantized(pathToImage, q.data(), W, H);
  }
  return CRT_OK;
}

std::vector<std::vector<Color>> RayTracer::render(const std::string &pathToImage, RenderOptions ro) {
  const unsigned int W = scene.sceneSettings.image.width, H = scene.sceneSettings.image.height;
  int rc = renderFlat(pathToImage, ro, frame.data());
  if (rc != CRT_OK) throw std::runtime_error(std::string("render failed: ") + (multi ? crt_multi_last_error(multi) : crt_last_error(ctx)));
  std::vector<std::vector<Color>> colorBuffer(H, std::vector<Color>(W));
  for (unsigned int y = 0; y < H; y++)
    for (unsigned int x = 0; x < W; x++) {
      const float *p = &frame[((size_t)y * W + x) * 3];
      colorBuffer[y][x] = Color(p[0], p[1], p[2]);
    }
  return colorBuffer;
}

std::vector<std::vector<Color>> RayTracer::renderProgressive(const std::string &pathToImage, RenderOptions ro, unsigned int samplesPerCall) {
  if (multi) throw std::runtime_error("renderProgressive: not available on a multi-device tracer");
  const unsigned int W = scene.sceneSettings.image.width, H = scene.sceneSettings.image.height;
  crt_options o{};
  o.max_depth = ro.MAX_DEPTH;
  o.shadow_bias = ro.SHADOW_BIAS;
  o.reflection_bias = ro.REFLECTION_BIAS;
  o.refraction_bias = ro.REFRACTION_BIAS;
  o.use_gi = ro.USE_GI ? 1u : 0u;
  o.gi_sample_size = ro.GI_SAMPLE_SIZE;
  o.monte_carlo_bias = ro.MONTE_CARLO_BIAS;
  o.gi_seed = ro.USE_GI ? giSeed++ : 0u;  // as renderFlat takes it
  const unsigned int samples = ro.RAYS_PER_PIXEL ? ro.RAYS_PER_PIXEL : 1u;  // (0 renders like 1, as in the reference)
  samplesPerCall = std::min(std::max(samplesPerCall, 1u), samples);
  const Matrix3 &m = camera.getRotationMatrix();
  const float pos[3] = {camera.getPosition().x, camera.getPosition().y, camera.getPosition().z};
  int rc = crt_set_camera(ctx, pos, &m.m[0][0]);  // (starts a new frame)
  for (unsigned int done = 0; rc == CRT_OK && done < samples;) {
    const unsigned int k = std::min(samplesPerCall, samples - done);
    rc = crt_render_progressive(ctx, &o, done, k, done + k == samples ? frame.data() : nullptr);  // the host copy of the last call's mean only
    done += k;
  }
  if (rc == CRT_OK && !pathToImage.empty()) {
    std::vector<uint8_t> q((size_t)W * H * 3);
    rc = crt_read_quantized(ctx, q.data());
    if (rc == CRT_OK) writePPMQuantized(pathToImage, q.data(), W, H);
  }
  if (rc != CRT_OK) throw std::runtime_error(std::string("renderProgressive failed: ") + crt_last_error(ctx));
  std::vector<std::vector<Color>> colorBuffer(H, std::vector<Color>(W));
  for (unsigned int y = 0; y < H; y++)
    for (unsigned int x = 0; x < W; x++) {
      const float *p = &frame[((size_t)y * W + x) * 3];
      colorBuffer[y][x] = Color(p[0], p[1], p[2]);
    }
  return colorBuffer;
}

std::vector<std::vector<Color>> RayTracer::renderAdaptive(const std::string &pathToImage, RenderOptions ro, const crt_adaptive &adaptive,
                                                          unsigned int passesPerCall, std::vector<uint32_t> *counts, bool split) {
  if (multi) throw std::runtime_error("renderAdaptive: not available on a multi-device tracer");
  const unsigned int W = scene.sceneSettings.image.width, H = scene.sceneSettings.image.height;
  crt_options o{};
  o.max_depth = ro.MAX_DEPTH;
  o.shadow_bias = ro.SHADOW_BIAS;
  o.reflection_bias = ro.REFLECTION_BIAS;
  o.refraction_bias = ro.REFRACTION_BIAS;
  o.use_gi = ro.USE_GI ? 1u : 0u;
  o.gi_sample_size = ro.GI_SAMPLE_SIZE;
  o.monte_carlo_bias = ro.MONTE_CARLO_BIAS;
  o.gi_seed = ro.USE_GI ? giSeed++ : 0u;  // as renderFlat takes it
  passesPerCall = std::max(passesPerCall, 1u);
  std::vector<uint32_t> held((size_t)W * H, 0u);
  const Matrix3 &m = camera.getRotationMatrix();
  const float pos[3] = {camera.getPosition().x, camera.getPosition().y, camera.getPosition().z};
  int rc = crt_set_camera(ctx, pos, &m.m[0][0]);  // (starts a new frame)
  for (unsigned int done = 0; rc == CRT_OK && (done == 0 || (done < adaptive.max_samples && crt_progressive_active(ctx)));) {
    const unsigned int k = std::min(passesPerCall, std::max(adaptive.max_samples, 1u) - done);
    rc = (split ? crt_render_adaptive_split : crt_render_adaptive)(ctx, &o, &adaptive, done, k, frame.data(), held.data());
    done += k;
  }
  if (rc == CRT_OK && !pathToImage.empty()) {
    std::vector<uint8_t> q((size_t)W * H * 3);
    rc = crt_read_quantized(ctx, q.data());
    if (rc == CRT_OK) writePPMQuantized(pathToImage, q.data(), W, H);
  }
  if (rc != CRT_OK) throw std::runtime_error(std::string("renderAdaptive failed: ") + crt_last_error(ctx));
  if (counts) counts->swap(held);
  std::vector<std::vector<Color>> colorBuffer(H, std::vector<Color>(W));
  for (unsigned int y = 0; y < H; y++)
    for (unsigned int x = 0; x < W; x++) {
      const float *p = &frame[((size_t)y * W + x) * 3];
      colorBuffer[y][x] = Color(p[0], p[1], p[2]);
    }
  return colorBuffer;
}

std::vector<std::vector<Color>> RayTracer::renderDenoised(const std::string &pathToImage, const crt_denoise &denoise, bool split) {
  if (multi) throw std::runtime_error("renderDenoised: not available on a multi-device tracer");
  const unsigned int W = scene.sceneSettings.image.width, H = scene.sceneSettings.image.height;
  std::vector<float> denoised((size_t)W * H * 3, 0.0f);
  std::vector<uint8_t> q(pathToImage.empty() ? 0 : (size_t)W * H * 3);
  const int rc = (split ? crt_render_denoised_split : crt_render_denoised)(ctx, &denoise, denoised.data(), pathToImage.empty() ? nullptr : q.data());
  if (rc != CRT_OK) throw std::runtime_error(std::string("renderDenoised failed: ") + crt_last_error(ctx));
  if (!pathToImage.empty()) writePPMQuantized(pathToImage, q.data(), W, H);
  std::vector<std::vector<Color>> colorBuffer(H, std::vector<Color>(W));
  for (unsigned int y = 0; y < H; y++)
    for (unsigned int x = 0; x < W; x++) {
      const float *p = &denoised[((size_t)y * W + x) * 3];
      colorBuffer[y][x] = Color(p[0], p[1], p[2]);
    }
  return colorBuffer;
}

std::vector<std::vector<Color>> RayTracer::renderAccumulated(const std::string &pathToImage, const crt_temporal &temporal, const crt_denoise *denoise,
                                                             double *validShare, bool split) {
  if (multi) throw std::runtime_error("renderAccumulated: not available on a multi-device tracer");
  const unsigned int W = scene.sceneSettings.image.width, H = scene.sceneSettings.image.height;
  std::vector<float> merged((size_t)W * H * 3, 0.0f);
  std::vector<uint8_t> q(pathToImage.empty() ? 0 : (size_t)W * H * 3);
  std::vector<uint8_t> valid(validShare ? (size_t)W * H : 0);
  const int rc = (split ? crt_render_accumulated_split : crt_render_accumulated)(ctx, &temporal, denoise, merged.data(), pathToImage.empty() ? nullptr : q.data(),
                                                                                 validShare ? valid.data() : nullptr);
  if (rc != CRT_OK) throw std::runtime_error(std::string("renderAccumulated failed: ") + crt_last_error(ctx));
  if (validShare) {  // over the hit pixels: the first hits of the camera's rays, which are the call's own guides
    std::vector<crt_hit> hits((size_t)W * H);
    crt_ray *rays = static_cast<crt_ray *>(crt_alloc_pinned((hits.size() ? hits.size() : 1) * sizeof(crt_ray)));
    if (!rays) throw std::runtime_error("out of pinned host memory");
    int qc = crt_camera_rays_device(ctx, rays, nullptr);  // (the context's camera is the frame's: no crt_set_camera, which would end the frame)
    if (qc == CRT_OK) qc = crt_synchronize(ctx);
    if (qc == CRT_OK) qc = crt_trace_rays(ctx, rays, hits.size(), CRT_RAY_PRIMARY, hits.data());
    crt_free_pinned(rays);
    if (qc != CRT_OK) throw std::runtime_error(std::string("renderAccumulated failed: ") + crt_last_error(ctx));
    size_t hit = 0, kept = 0;
    for (size_t i = 0; i < hits.size(); i++)
      if (hits[i].hit) { hit++; kept += valid[i] != 0; }
    *validShare = hit ? (double)kept / (double)hit : 0.0;
  }
  if (!pathToImage.empty()) writePPMQuantized(pathToImage, q.data(), W, H);
  std::vector<std::vector<Color>> colorBuffer(H, std::vector<Color>(W));
  for (unsigned int y = 0; y < H; y++)
    for (unsigned int x = 0; x < W; x++) {
      const float *p = &merged[((size_t)y * W + x) * 3];
      colorBuffer[y][x] = Color(p[0], p[1], p[2]);
    }
  return colorBuffer;
}

void RayTracer::resetHistory() {
  if (multi) throw std::runtime_error("resetHistory: not available on a multi-device tracer");
  if (crt_history_reset(ctx) != CRT_OK) throw std::runtime_error("resetHistory failed");
}

void RayTracer::exportPPM(const std::string &pathToImage, const std::vector<std::vector<Color>> &colorBuffer) {
  const unsigned int W = scene.sceneSettings.image.width, H = scene.sceneSettings.image.height;
  std::vector<float> flatRGB((size_t)W * H * 3, 0.0f);
  for (unsigned int y = 0; y < H && y < colorBuffer.size(); y++)
    for (unsigned int x = 0; x < W && x < colorBuffer[y].size(); x++) {
      flatRGB[((size_t)y * W + x) * 3 + 0] = colorBuffer[y][x].x;
      flatRGB[((size_t)y * W + x) * 3 + 1] = colorBuffer[y][x].y;
      flatRGB[((size_t)y * W + x) * 3 + 2] = colorBuffer[y][x].z;
    }
  writePPM(pathToImage, flatRGB.data(), W, H);
}

}  // namespace crt
