// crt::RayTracer -- the seam.  Same public surface as the reference's class
// (reference: SourceCode/include/tracer/RayTracer.h:12-50,96-101):
//     explicit RayTracer(Scene&);  getCamera();  setCamera();
//     std::vector<std::vector<Color>> render(const std::string& pathToImage, RenderOptions = RenderOptions());
//     void exportPPM(const std::string&, const std::vector<std::vector<Color>>&);
// The per-pixel work (renderRectangle -> getRay -> shootRay -> ...) runs on the MI355X through the C
// ABI of include/crt_hip.h; scheduling (the std::thread pools of RayTracer.cpp:114-202) is replaced by
// the GPU's own pixel queue, but WHICH pixels a render covers is still decided by the reference's bucket
// arithmetic (RayTracer.cpp:141-152), because that is observable in the output.
#pragma once

#include <string>
#include <vector>

#include "../../include/crt_hip.h"
#include "AccelerationStructure.h"
#include "Scene.h"

namespace crt {

enum RenderOptimization {  // RayTracer.h:12-23
  NoOptimization,
  Regions,
  BucketsThreadPool,
  BucketsQueue,
  AABB,
  BucketsThreadPoolAABB,
  BucketsQueueAABB,
  BVH,
  BVHBucketsThreadPool,
  BVHBucketsQueue
};

struct RenderOptions {  // RayTracer.h:25-50, same fields, defaults and constructor order
  RenderOptimization optimization = BVHBucketsThreadPool;
  bool USE_GI = false;
  unsigned int MAX_DEPTH = 5;
  unsigned int GI_SAMPLE_SIZE = 2;
  unsigned int RAYS_PER_PIXEL = 1;
  float SHADOW_BIAS = 1e-4;
  float REFLECTION_BIAS = 1e-4;
  float REFRACTION_BIAS = 1e-4;
  float MONTE_CARLO_BIAS = 1e-4;

  explicit RenderOptions(const RenderOptimization optimization = BVHBucketsThreadPool, const unsigned int maxDepth = 5,
                         const bool useGI = false, const unsigned int sampleSize = 2, const unsigned int raysPerPixel = 1,
                         const float shadowBias = 1e-4, const float reflectionBias = 1e-4,
                         const float refractionBias = 1e-4, const float monteCarloBias = 1e-4)
      : optimization{optimization}, USE_GI{useGI}, MAX_DEPTH{maxDepth}, GI_SAMPLE_SIZE{sampleSize},
        RAYS_PER_PIXEL{raysPerPixel}, SHADOW_BIAS{shadowBias}, REFLECTION_BIAS{reflectionBias},
        REFRACTION_BIAS{refractionBias}, MONTE_CARLO_BIAS{monteCarloBias} {}
};

// The rectangles RayTracer::render hands to renderRectangle for a given optimisation mode
// (RayTracer.cpp:209-286 + renderRegions :114-139 / renderBucketsThreadpool :141-158 / renderBucketsQueue
// :160-202; the queue variant shuffles the same set).  `hardwareConcurrency` stands for
// std::thread::hardware_concurrency() (used by the Regions mode only).
std::vector<crt_rect> bucketRectangles(unsigned int width, unsigned int height, unsigned int bucketSize,
                                       RenderOptimization optimization, unsigned int hardwareConcurrency);

// P3 writer, byte-identical to RayTracer::exportPPM + PPMColor (RayTracer.cpp:540-552, Color.cpp:12-21).
void writePPM(const std::string &path, const float *rgb, unsigned int width, unsigned int height);
void writePPMQuantized(const std::string &path, const uint8_t *rgb8, unsigned int width, unsigned int height);

class RayTracer {
 public:
  // Builds the two-level tree once (as RayTracer::RayTracer does, RayTracer.cpp:45-51), flattens it and
  // uploads scene + tree to the GPU.  Throws std::runtime_error when no usable GPU exists: there is no
  // CPU fallback.
  explicit RayTracer(Scene &scene, int device = 0, const crt_tuning *tuning = nullptr);
  // The same on several GPUs of one node: the frame's 8x8 tiles are dealt over `devices`, gathered on devices[0]
  // (crt_hip.h: crt_multi).  This is what replaces the reference's thread pool over buckets (RayTracer.cpp:141-158).
  RayTracer(Scene &scene, const std::vector<int> &devices, const crt_tuning *tuning = nullptr);
  ~RayTracer();
  RayTracer(const RayTracer &) = delete;
  RayTracer &operator=(const RayTracer &) = delete;

  const Camera &getCamera() const { return camera; }
  Camera &setCamera() { return camera; }
  std::vector<std::vector<Color>> render(const std::string &pathToImage, RenderOptions renderOptions = RenderOptions());
  void exportPPM(const std::string &pathToImage, const std::vector<std::vector<Color>> &colorBuffer);

  // ---- frames in flight (animation: app/animation.cpp:24-38 renders frame after frame with a new camera each).
  // setFramesInFlight(k) keeps the scene resident in k contexts; renderAsync() enqueues a frame with the CURRENT camera on
  // the next one and returns its slot at once; finishFrame(slot) waits for that frame and returns its quantised pixels
  // (H*W*3 bytes, PPMColor rule, valid until the slot is used again).  The GPU then works on frame k+1's primary rays while
  // frame k's deepest recursion levels and its copy to the host drain.  render() is unaffected.
  // USE_GI frames (RayTracer.cpp:90-104, 331-354): the reference seeds its generator from clock() ^ thread id, so no two of its
  // renders agree; here frame k of a tracer uses seed k (csrc/gi_random.h) unless setGISeed() says otherwise
  void setGISeed(unsigned int seed) { giSeed = seed; }
  void setFramesInFlight(unsigned int k);
  unsigned int framesInFlight() const { return (unsigned int)ring.size(); }
  int renderAsync(const RenderOptions &renderOptions);
  const uint8_t *finishFrame(int slot);

  // ---- ray queries (crt_hip.h: crt_trace_rays / crt_occluded_rays): what AccelerationStructure::intersect and
  // AccelerationStructure::checkForIntersection (KDTree.cpp:127-192, AccelerationStructure.cpp:56-94) answer for rays of the
  // caller's -- directions as given, exact for every ray.  Single-device tracers only (std::runtime_error otherwise).
  std::vector<crt_hit> traceRays(const std::vector<crt_ray> &rays, unsigned int rayType = CRT_RAY_REFLECTION);
  std::vector<unsigned char> occludedRays(const std::vector<crt_ray> &rays, const std::vector<float> &maxDistance);
  // RayTracer::getRay (RayTracer.cpp:61-80) at every pixel centre with the CURRENT camera, row-major
  std::vector<crt_ray> cameraRays();
  crt_query_stats queryStats() const;
  // ---- direct lighting (crt_hip.h: crt_shade_hits / crt_light_points): what shootRay returns for a ray whose closest hit is hits[i]
  // wherever it does not recurse -- calculateDiffusion (RayTracer.cpp:300-330) for a diffuse hit, the background for none --, 3 floats
  // per record, CRT_SHADE_* per record in *status when it is given; and the lights' unoccluded factors summed at points of the caller's
  std::vector<float> shadeHits(const std::vector<crt_hit> &hits, float shadowBias = 1e-4f, std::vector<unsigned char> *status = nullptr);
  std::vector<float> lightPoints(const std::vector<float> &points, const std::vector<float> &normals, float shadowBias = 1e-4f);
  // ---- radiance queries (crt_hip.h: crt_shoot_rays): what shootRay(Ray{origin, direction, rayType}, 0) returns for rays of the
  // caller's -- the direction normalised on entry, reflections, refractions and the Fresnel mix down to renderOptions.MAX_DEPTH, the
  // three biases from renderOptions (USE_GI is refused) --, 3 floats per ray; *stats: the call's crt_shoot_stats when it is given
  std::vector<float> shootRays(const std::vector<crt_ray> &rays, const RenderOptions &renderOptions, unsigned int rayType = CRT_RAY_REFLECTION,
                               crt_shoot_stats *stats = nullptr);
  // ... and in the GI mode (crt_hip.h: crt_shoot_rays_gi): shootRay of the GI build with the generator of csrc/gi_random.h; keys: one
  // per ray, or empty for the keys of a frame's pixels 0 .. n - 1, sample 0, under the tracer's seed (setGISeed).  MAX_DEPTH,
  // GI_SAMPLE_SIZE and the four biases come from renderOptions; USE_GI must be set, RAYS_PER_PIXEL is not read
  std::vector<float> shootRaysGI(const std::vector<crt_ray> &rays, const std::vector<uint32_t> &keys, const RenderOptions &renderOptions,
                                 unsigned int rayType = CRT_RAY_REFLECTION, crt_shoot_stats *stats = nullptr);

  // ---- lightmap baking (crt_hip.h: "Lightmap baking", crt_bake_lightmap): the bake.width x bake.height lightmap of mesh bake.mesh's UV layout,
  // row 0 the top, 3 floats per texel: every covered texel is what shootRay returns for its probe ray -- MAX_DEPTH and the biases from
  // renderOptions; with USE_GI the mean of bake.samples GI samples of GI_SAMPLE_SIZE rays per hit under the tracer's seed (setGISeed) --,
  // the texels beside a chart filled by bake.dilate dilation passes.  pathToImage: the map as a PPM when it is not empty; *status: a byte a
  // texel (CRT_BAKE_EMPTY / COVERED / DILATED), *stats: the call's crt_bake_stats, when they are given.  Single-device tracers only.
  std::vector<float> bakeLightmap(const std::string &pathToImage, const crt_bake &bake, const RenderOptions &renderOptions,
                                  std::vector<unsigned char> *status = nullptr, crt_bake_stats *stats = nullptr);

  // ---- irradiance probes (crt_hip.h: "Irradiance probes", crt_bake_probes, crt_probe_irradiance): bakeProbes gives the volume's nx * ny * nz
  // SH9 records, each the projection of what shootRay returns for the probe's rays -- MAX_DEPTH and the biases from renderOptions; with USE_GI
  // the GI mode of GI_SAMPLE_SIZE rays per hit under the VOLUME's gi_seed --, *stats the call's crt_probe_stats.  probeIrradiance gives the
  // light a white Lambertian surface shows at the points (3 floats each) with the normals, 3 floats per point, *status the corners used
  // (0: no light).  probeIrradianceView is the volume seen by the camera: every pixel's camera ray is traced, a hit is looked up at its point
  // with its normal, a miss or a lookup without light is the background; pathToImage: the view as a PPM when it is not empty.
  // Single-device tracers only.
  std::vector<crt_probe> bakeProbes(const crt_probe_volume &volume, const RenderOptions &renderOptions, crt_probe_stats *stats = nullptr);
  std::vector<float> probeIrradiance(const crt_probe_volume &volume, const std::vector<crt_probe> &probes, const std::vector<float> &points,
                                     const std::vector<float> &normals, std::vector<unsigned char> *status = nullptr);
  std::vector<float> probeIrradianceView(const std::string &pathToImage, const crt_probe_volume &volume, const std::vector<crt_probe> &probes,
                                         const crt_probe_visibility *visibility = nullptr, const std::vector<crt_probe_depth> *depth = nullptr);

  // ---- probe visibility (crt_hip.h: "Probe visibility", crt_bake_probes_visible, crt_probe_irradiance_visible): bakeProbesVisible is
  // bakeProbes with the depth pass -- *depth takes the volume's nx * ny * nz depth records --, and probeIrradianceVisible is probeIrradiance
  // with every corner weighted by the Chebyshev bound of its depth record.  probeIrradianceView with a visibility and depth records looks the
  // camera rays' first hits up that way.  Single-device tracers only.
  std::vector<crt_probe> bakeProbesVisible(const crt_probe_volume &volume, const crt_probe_visibility &visibility, const RenderOptions &renderOptions,
                                           std::vector<crt_probe_depth> *depth, crt_probe_stats *stats = nullptr);
  std::vector<float> probeIrradianceVisible(const crt_probe_volume &volume, const crt_probe_visibility &visibility, const std::vector<crt_probe> &probes,
                                            const std::vector<crt_probe_depth> &depth, const std::vector<float> &points, const std::vector<float> &normals,
                                            std::vector<unsigned char> *status = nullptr);

  // ---- probe-lit radiance (crt_hip.h: "Probe-lit radiance", crt_shoot_rays_lit, crt_render_probe_lit): shootRaysLit is shootRaysGI with
  // the probe volume in place of the sample rays -- a diffuse hit takes GI_SAMPLE_SIZE times the volume's zonal lookup at its point and
  // normal as its indirect sum, through mirrors and glass too; renderProbeLit is that for the camera's rays of every pixel, written as a
  // PPM when pathToImage is not empty, *stats the frame's lit and unlit records.  renderOptions.USE_GI is taken as set.  A visibility
  // needs the depth records.  Single-device tracers only.
  std::vector<float> shootRaysLit(const std::vector<crt_ray> &rays, unsigned rayType, const RenderOptions &renderOptions, const crt_probe_volume &volume,
                                  const std::vector<crt_probe> &probes, const crt_probe_visibility *visibility = nullptr,
                                  const std::vector<crt_probe_depth> *depth = nullptr);
  std::vector<float> renderProbeLit(const std::string &pathToImage, const RenderOptions &renderOptions, const crt_probe_volume &volume,
                                    const std::vector<crt_probe> &probes, const crt_probe_visibility *visibility = nullptr,
                                    const std::vector<crt_probe_depth> *depth = nullptr, crt_probe_lit_stats *stats = nullptr);

  // ---- chain guides (crt_hip.h: "Chain guides", crt_guide_rays): for every ray the guide record of the surface it shows -- the chain of
  // closest hits through reflective and refractive meshes to the first diffuse or constant surface, a miss or maxBounces (<= 63) --, with
  // the path length as t and a tagged mesh; the biases come from renderOptions.  *status: a byte a ray (bits 0-5 the bounces, bit 7 cut),
  // *lastRays: the terminal segment's ray, when they are given.  Single-device tracers only.
  std::vector<crt_hit> guideRays(const std::vector<crt_ray> &rays, const RenderOptions &renderOptions, unsigned int maxBounces,
                                 unsigned int rayType = CRT_RAY_PRIMARY, std::vector<unsigned char> *status = nullptr,
                                 std::vector<crt_ray> *lastRays = nullptr);
  // 0 (the default): renderDenoised and renderAccumulated filter under first-hit guides; above 0: under the chain guides of the camera's
  // centre rays (crt_set_guide_bounces); the temporal stage keeps the first hits
  void setGuideBounces(unsigned int maxBounces);
  unsigned int guideBounces() const;
  // null (the default): off; otherwise renderDenoised and renderAccumulated (with a filter) estimate the variance of pixels whose moments
  // stand for fewer than estimate->min_history samples from their 7x7 neighbourhood before the filter (crt_set_variance_estimate)
  void setVarianceEstimate(const crt_variance_estimate *estimate);

  // ---- progressive GI frames (crt_hip.h: crt_render_progressive): render()'s USE_GI frame with renderOptions.RAYS_PER_PIXEL rays per
  // pixel, samplesPerCall samples a call, in memory that does not depend on RAYS_PER_PIXEL; the frame's seed is taken as render() takes
  // it.  EVERY pixel of the frame is rendered: where render()'s bucket grid covers the frame (RayTracer.cpp:141-152 can leave edge rows
  // out) the PPM is render()'s byte for byte.  Single-device tracers only; USE_GI must be set.
  std::vector<std::vector<Color>> renderProgressive(const std::string &pathToImage, RenderOptions renderOptions, unsigned int samplesPerCall = 1);

  // ---- adaptive sampling (crt_hip.h: crt_render_adaptive): that frame with every pixel shot until the rule of `adaptive` stops it, at most
  // adaptive.max_samples times (RAYS_PER_PIXEL is not read), passesPerCall passes a call; the calls end when no pixel is left.  counts, if
  // given, receives the samples each pixel holds (row-major): a pixel with k samples is render()'s pixel with RAYS_PER_PIXEL = k.
  // Single-device tracers only; USE_GI must be set.
  std::vector<std::vector<Color>> renderAdaptive(const std::string &pathToImage, RenderOptions renderOptions, const crt_adaptive &adaptive,
                                                 unsigned int passesPerCall = 1, std::vector<uint32_t> *counts = nullptr, bool split = false);

  // ---- denoising (crt_hip.h: crt_render_denoised): the adaptive frame renderAdaptive left, under way or finished, through the
  // variance-guided a-trous filter with the settings of `denoise` (crt_denoise_defaults), guided by the first hits of the camera's rays.
  // The frame itself is left as it was.  The PPM, if a path is given, is the denoised frame quantised by the PPMColor rule.
  // Single-device tracers only.
  // split (crt_hip.h: "Split GI frames"; all three calls): renderAdaptive keeps every sample's direct light beside the same frame, and
  // renderDenoised / renderAccumulated filter and reproject the indirect light only and add the direct light -- the texels -- back.
  std::vector<std::vector<Color>> renderDenoised(const std::string &pathToImage, const crt_denoise &denoise, bool split = false);

  // ---- temporal accumulation (crt_hip.h: crt_render_accumulated): the adaptive frame renderAdaptive left, merged with the history of the
  // frames accumulated before it -- reprojected through the camera each of them had -- and then, with `denoise`, through the a-trous
  // filter (nullptr: no spatial filter).  The frame itself is left as it was; the history survives setCamera().  Give consecutive frames
  // different gi seeds.  validShare, if given, receives the share of the hit pixels with at least one valid history tap.  The PPM, if
  // a path is given, is the result quantised by the PPMColor rule.  Single-device tracers only.
  std::vector<std::vector<Color>> renderAccumulated(const std::string &pathToImage, const crt_temporal &temporal, const crt_denoise *denoise = nullptr,
                                                    double *validShare = nullptr, bool split = false);
  void resetHistory();

  // flat access for callers that do not want the vector-of-vectors copy
  int renderFlat(const std::string &pathToImage, const RenderOptions &renderOptions, float *outRGB, unsigned int counters = 0);
  crt_ctx *context() const { return multi ? crt_multi_context(multi, 0) : ctx; }
  crt_multi *multiContext() const { return multi; }
  const FlatScene &flatScene() const { return flat; }
  const AccelerationStructure &acceleration() const { return accelerationStructure; }
  crt_stats stats() const;
  // What the last render did differently from the reference, in words ("" when nothing): the reference's seven non-tree
  // RenderOptimization modes (brute force, single AABB) accept a handful of hits its tree modes drop; every mode renders
  // with the TREE's semantics here, the mode only selects the pixel coverage -- a caller that asks for one of them is told so.
  const std::string &renderNote() const { return note; }

 private:
  std::string note;
  const AccelerationStructure accelerationStructure;
  const Scene &scene;
  Camera camera;
  FlatScene flat;
  crt_ctx *ctx = nullptr;
  crt_multi *multi = nullptr;  // set instead of ctx when the tracer was built for several devices
  struct InFlight { crt_ctx *ctx = nullptr; uint8_t *rgb8 = nullptr; bool busy = false; };
  std::vector<InFlight> ring;  // ring[0].ctx == ctx
  unsigned int ringNext = 0;
  unsigned int giSeed = 0;
  int deviceIndex = 0;
  crt_tuning tuningCopy{};
  bool haveTuning = false;
  std::vector<float> frame;  // persistent colorBuffer (RayTracer.h:69)
};

}  // namespace crt
