// crt_main -- still-image driver.  Replaces the reference's app/main.cpp (which hard-codes
// /home/daniel paths, app/main.cpp:12,16) with the same flow taking its paths from the command line:
//   parse scene -> RayTracer(scene) -> render(path, options) -> PPM.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../host/RayTracer.h"
#include "../host/SceneParser.h"

int main(int argc, char **argv) {
  if (argc < 3) {
    std::fprintf(stderr,
                 "usage: %s scene.crtscene out.ppm [--folder DIR] [--depth N] [--mode 0..9] [--device D | --devices 0-7 | --devices 0,2,5] [--repeat K]\n"
                 "       [--gi GI_SAMPLE_SIZE RAYS_PER_PIXEL [--seed S] [--progressive K]]   (RenderOptions::USE_GI, RayTracer.h:27-30;\n"
                 "        --progressive: the same frame K samples a call, in memory that does not depend on RAYS_PER_PIXEL)\n"
                 "       [--gi GI_SAMPLE_SIZE RAYS_PER_PIXEL --adaptive THRESHOLD MIN MAX [--counts FILE]]   (every pixel is shot until the rule of\n"
                 "        crt_hip.h's crt_adaptive stops it, MIN .. MAX times; RAYS_PER_PIXEL is not read; --counts: the samples per pixel as a P2 PGM)\n"
                 "       [--gi GI_SAMPLE_SIZE RAYS_PER_PIXEL --adaptive THRESHOLD MIN MAX --denoise [ITERATIONS] [--split] [--guide-bounces B] [--variance-estimate [MIN_HISTORY]]]   (out.ppm is that frame through\n"
                 "        the variance-guided a-trous filter of crt_hip.h's crt_denoise, its defaults but for ITERATIONS, 0..8; --split: the filter acts\n"
                 "        on the indirect light only and the direct light is added back, crt_hip.h's \"Split GI frames\"; it needs --adaptive;\n"
                 "        --guide-bounces B, 0..63: the filter runs under guides that follow mirrors and glass for up to B bounces, crt_hip.h's \"Chain guides\";\n"
                 "        it needs --denoise;\n"
                 "        --variance-estimate [MIN_HISTORY]: a pixel whose moments stand for fewer samples gets a 7x7 estimate of its variance before the\n"
                 "        filter, crt_hip.h's \"Variance estimate\", its defaults but for MIN_HISTORY; it needs --denoise)\n"
                 "       [--probe ROW COL]   (no render: the closest hit of that pixel's camera ray; out.ppm is not written)\n"
                 "       [--bake MESH WIDTH HEIGHT [--gi GI_SAMPLE_SIZE SAMPLES_PER_TEXEL [--seed S]] [--dilate K] [--probe-offset X]]   (no render: out.ppm is the\n"
                 "        WIDTH x HEIGHT lightmap of that mesh's UV layout, crt_hip.h's \"Lightmap baking\", its defaults but for what is given; one device)\n"
                 "       [--probes OX OY OZ SX SY SZ NX NY NZ [--probe-rays R] [--gi GI_SAMPLE_SIZE 1 [--seed S]] [--backface-limit X] [--probes-out FILE]]   (no\n"
                 "        render: bakes the NX x NY x NZ irradiance probe volume at origin O with spacing S, crt_hip.h's \"Irradiance probes\"; out.ppm is the\n"
                 "        volume seen by the camera: a hit pixel is the lookup at its point with its normal, every other pixel the background; FILE: the raw\n"
                 "        128-byte records; one device;\n"
                 "        --probe-visibility [MAX_DISTANCE] [--probe-depth-out FILE]: crt_hip.h's \"Probe visibility\": the bake also makes the depth records,\n"
                 "        with the volume's default parameters but for MAX_DISTANCE, and out.ppm is the Chebyshev-weighted lookup; FILE: the raw 512-byte depth\n"
                 "        records; it needs --probes;\n"
                 "        --probe-lit [S]: crt_hip.h's \"Probe-lit radiance\": the volume is baked with --depth minus one, and out.ppm is the frame of the\n"
                 "        radiance queries -- direct light, mirrors and glass -- whose diffuse hits take S (default: GI_SAMPLE_SIZE) times the volume's zonal\n"
                 "        lookup as their indirect sum; it needs --probes and --gi GI_SAMPLE_SIZE 1)\n",
                 argv[0]);
    return 2;
  }
  std::string scenePath = argv[1], outPath = argv[2], folder;
  unsigned depth = 5;
  int mode = crt::BVHBucketsThreadPool, device = 0, repeat = 1;
  std::vector<int> devices;  // --devices: the frame's tiles over several GPUs (first one gathers)
  bool useGI = false;
  unsigned giSamples = 2, raysPerPixel = 1, seed = 0, progressive = 0;
  bool adaptive = false;
  float adaptiveThreshold = 0.0f;
  unsigned adaptiveMin = 0, adaptiveMax = 0;
  std::string countsPath;
  bool denoise = false;
  int denoiseIterations = -1;  // (-1: crt_denoise_defaults')
  bool split = false;
  int guideBounces = -1;  // (-1: not given)
  bool varianceEstimate = false;
  float minHistory = -1.0f;  // (-1: crt_variance_estimate_defaults')
  bool probe = false;
  unsigned probeRow = 0, probeCol = 0;
  bool bake = false;
  unsigned bakeMesh = 0, bakeWidth = 0, bakeHeight = 0;
  bool dilateGiven = false, probeOffsetGiven = false;   // (not given: crt_bake_defaults')
  long long bakeDilate = 0;
  float probeOffset = 0.0f;
  bool probes = false, backfaceLimitGiven = false;
  crt_probe_volume volume;
  crt_probe_volume_defaults(&volume);
  long long probeRays = -1;   // (-1: crt_probe_volume_defaults')
  std::string probesOut, probeDepthOut;
  bool probeVisibility = false, probeMaxDistanceGiven = false;
  float probeMaxDistance = 0.0f;
  bool probeLit = false;
  long long probeLitSamples = -1;   // (-1: GI_SAMPLE_SIZE)
  for (int i = 3; i < argc; i++) {
    if (!strcmp(argv[i], "--folder") && i + 1 < argc) folder = argv[++i];
    else if (!strcmp(argv[i], "--depth") && i + 1 < argc) depth = (unsigned)atoi(argv[++i]);
    else if (!strcmp(argv[i], "--mode") && i + 1 < argc) mode = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--device") && i + 1 < argc) device = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--devices") && i + 1 < argc) {
      const char *p = argv[++i];
      while (*p) {
        char *end = nullptr;
        long a = strtol(p, &end, 10), b = a;
        if (end == p) break;
        if (*end == '-') { p = end + 1; b = strtol(p, &end, 10); if (end == p) break; }
        for (long d = a; d <= b && devices.size() < 64; d++) devices.push_back((int)d);
        p = (*end == ',') ? end + 1 : end;
        if (*end && *end != ',') break;
      }
    }
    else if (!strcmp(argv[i], "--repeat") && i + 1 < argc) repeat = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--gi") && i + 2 < argc) { useGI = true; giSamples = (unsigned)atoi(argv[++i]); raysPerPixel = (unsigned)atoi(argv[++i]); }
    else if (!strcmp(argv[i], "--seed") && i + 1 < argc) seed = (unsigned)strtoul(argv[++i], nullptr, 0);
    else if (!strcmp(argv[i], "--progressive") && i + 1 < argc) progressive = (unsigned)atoi(argv[++i]);
    else if (!strcmp(argv[i], "--adaptive") && i + 3 < argc) {
      adaptive = true; adaptiveThreshold = (float)atof(argv[++i]); adaptiveMin = (unsigned)atoi(argv[++i]); adaptiveMax = (unsigned)atoi(argv[++i]);
    }
    else if (!strcmp(argv[i], "--counts") && i + 1 < argc) countsPath = argv[++i];
    else if (!strcmp(argv[i], "--denoise")) {
      denoise = true;
      if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') denoiseIterations = atoi(argv[++i]);
    }
    else if (!strcmp(argv[i], "--split")) split = true;
    else if (!strcmp(argv[i], "--guide-bounces") && i + 1 < argc) guideBounces = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--variance-estimate")) {
      varianceEstimate = true;
      if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') minHistory = (float)atof(argv[++i]);
    }
    else if (!strcmp(argv[i], "--bake") && i + 3 < argc) {
      bake = true; bakeMesh = (unsigned)atoi(argv[++i]); bakeWidth = (unsigned)atoi(argv[++i]); bakeHeight = (unsigned)atoi(argv[++i]);
    }
    else if (!strcmp(argv[i], "--dilate") && i + 1 < argc) { dilateGiven = true; bakeDilate = atoll(argv[++i]); }
    else if (!strcmp(argv[i], "--probe-offset") && i + 1 < argc) { probeOffsetGiven = true; probeOffset = (float)atof(argv[++i]); }
    else if (!strcmp(argv[i], "--probes") && i + 9 < argc) {
      probes = true;
      for (int k = 0; k < 3; k++) volume.origin[k] = (float)atof(argv[++i]);
      for (int k = 0; k < 3; k++) volume.spacing[k] = (float)atof(argv[++i]);
      volume.nx = (uint32_t)strtoul(argv[++i], nullptr, 10); volume.ny = (uint32_t)strtoul(argv[++i], nullptr, 10); volume.nz = (uint32_t)strtoul(argv[++i], nullptr, 10);
    }
    else if (!strcmp(argv[i], "--probe-rays") && i + 1 < argc) probeRays = atoll(argv[++i]);
    else if (!strcmp(argv[i], "--backface-limit") && i + 1 < argc) { backfaceLimitGiven = true; volume.backface_limit = (float)atof(argv[++i]); }
    else if (!strcmp(argv[i], "--probes-out") && i + 1 < argc) probesOut = argv[++i];
    else if (!strcmp(argv[i], "--probe-visibility")) {
      probeVisibility = true;
      if (i + 1 < argc && argv[i + 1][0] != '-') { probeMaxDistanceGiven = true; probeMaxDistance = (float)atof(argv[++i]); }
    }
    else if (!strcmp(argv[i], "--probe-depth-out") && i + 1 < argc) probeDepthOut = argv[++i];
    else if (!strcmp(argv[i], "--probe-lit")) {
      probeLit = true;
      if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') probeLitSamples = atoll(argv[++i]);
    }
    else if (!strcmp(argv[i], "--probe") && i + 2 < argc) { probe = true; probeRow = (unsigned)atoi(argv[++i]); probeCol = (unsigned)atoi(argv[++i]); }
  }
  if (bake && (devices.size() > 0 || progressive || adaptive || denoise || probe)) {
    std::fprintf(stderr, "error: --bake needs one device and excludes --progressive, --adaptive, --denoise and --probe\n");
    return 2;
  }
  if (probes && (devices.size() > 0 || progressive || adaptive || denoise || probe || bake)) {
    std::fprintf(stderr, "error: --probes needs one device and excludes --progressive, --adaptive, --denoise, --probe and --bake\n");
    return 2;
  }
  if ((probeRays != -1 || backfaceLimitGiven || !probesOut.empty()) && !probes) {
    std::fprintf(stderr, "error: --probe-rays, --backface-limit and --probes-out need --probes\n");
    return 2;
  }
  if ((probeVisibility || !probeDepthOut.empty()) && !probes) {
    std::fprintf(stderr, "error: --probe-visibility and --probe-depth-out need --probes\n");
    return 2;
  }
  if (probeLit && (!probes || !useGI || probeLitSamples > 64)) {
    std::fprintf(stderr, "error: --probe-lit needs --probes and --gi GI_SAMPLE_SIZE 1, and an S of 0 .. 64\n");
    return 2;
  }
  if (!probeDepthOut.empty() && !probeVisibility) {
    std::fprintf(stderr, "error: --probe-depth-out needs --probe-visibility\n");
    return 2;
  }
  if (probeRays != -1 && (probeRays < 0 || probeRays > 0xFFFFFFFFll)) {
    std::fprintf(stderr, "error: --probe-rays takes a ray count\n");
    return 2;
  }
  if (dilateGiven && (bakeDilate < 0 || bakeDilate > 0xFFFFFFFFll)) {
    std::fprintf(stderr, "error: --dilate takes a pass count of 0 .. 4294967295\n");
    return 2;
  }
  if ((dilateGiven || probeOffsetGiven) && !bake) {
    std::fprintf(stderr, "error: --dilate and --probe-offset need --bake\n");
    return 2;
  }
  if (progressive && (!useGI || devices.size() > 0)) {
    std::fprintf(stderr, "error: --progressive needs --gi and one device\n");
    return 2;
  }
  if (adaptive && (!useGI || devices.size() > 0 || progressive)) {
    std::fprintf(stderr, "error: --adaptive needs --gi and one device, and excludes --progressive\n");
    return 2;
  }
  if (!countsPath.empty() && !adaptive) {
    std::fprintf(stderr, "error: --counts needs --adaptive\n");
    return 2;
  }
  if (denoise && !adaptive) {
    std::fprintf(stderr, "error: --denoise needs --adaptive\nusage: %s scene.crtscene out.ppm --gi GI_SAMPLE_SIZE RAYS_PER_PIXEL --adaptive THRESHOLD MIN MAX --denoise [ITERATIONS]\n",
                 argv[0]);
    return 2;
  }
  if (split && !adaptive) {
    std::fprintf(stderr, "error: --split needs --adaptive\nusage: %s scene.crtscene out.ppm --gi GI_SAMPLE_SIZE RAYS_PER_PIXEL --adaptive THRESHOLD MIN MAX --denoise [ITERATIONS] --split\n",
                 argv[0]);
    return 2;
  }
  if (guideBounces >= 0 && (!denoise || guideBounces > 63)) {
    std::fprintf(stderr, "error: --guide-bounces needs --denoise and a value of 0..63\nusage: %s scene.crtscene out.ppm --gi GI_SAMPLE_SIZE RAYS_PER_PIXEL --adaptive THRESHOLD MIN MAX --denoise [ITERATIONS] --guide-bounces B\n",
                 argv[0]);
    return 2;
  }
  if (varianceEstimate && !denoise) {
    std::fprintf(stderr, "error: --variance-estimate needs --denoise\nusage: %s scene.crtscene out.ppm --gi GI_SAMPLE_SIZE RAYS_PER_PIXEL --adaptive THRESHOLD MIN MAX --denoise [ITERATIONS] --variance-estimate [MIN_HISTORY]\n",
                 argv[0]);
    return 2;
  }
  try {
    crt::SceneParser parser;
    crt::Scene scene = parser.parseScene(scenePath, folder);
    auto t0 = std::chrono::high_resolution_clock::now();
    std::unique_ptr<crt::RayTracer> tracerPtr(devices.size() > 0 ? new crt::RayTracer(scene, devices) : new crt::RayTracer(scene, device));
    crt::RayTracer &tracer = *tracerPtr;
    auto t1 = std::chrono::high_resolution_clock::now();
    if (probe) {
      // picking: RayTracer::getRay at the pixel's centre (RayTracer.cpp:61-80), AccelerationStructure::intersect for it (KDTree.cpp:127-192)
      const unsigned W = scene.sceneSettings.image.width, H = scene.sceneSettings.image.height;
      if (probeRow >= H || probeCol >= W) { std::fprintf(stderr, "error: --probe %u %u is outside the %ux%u image\n", probeRow, probeCol, W, H); return 2; }
      const crt_ray ray = tracer.cameraRays()[(size_t)probeRow * W + probeCol];
      const crt_hit h = tracer.traceRays(std::vector<crt_ray>(1, ray), CRT_RAY_PRIMARY)[0];
      // (%a: the floats exactly)
      if (!h.hit) std::printf("probe row %u col %u: no hit\n", probeRow, probeCol);
      else std::printf("probe row %u col %u: mesh %u triangle %u t %a point %a %a %a normal %a %a %a\n", probeRow, probeCol, h.mesh, h.triangle,
                       (double)h.t, (double)h.point[0], (double)h.point[1], (double)h.point[2], (double)h.normal[0], (double)h.normal[1], (double)h.normal[2]);
      return 0;
    }
    crt::RenderOptions options((crt::RenderOptimization)mode, depth, useGI, giSamples, raysPerPixel);
    if (bake) {
      // the lightmap of a mesh's UV layout: with --gi N R, N GI samples per hit and R samples per texel
      crt_bake b;
      crt_bake_defaults(&b);
      b.mesh = bakeMesh; b.width = bakeWidth; b.height = bakeHeight;
      if (useGI) b.samples = raysPerPixel;
      if (dilateGiven) b.dilate = (uint32_t)bakeDilate;
      if (probeOffsetGiven) b.probe_offset = probeOffset;   // (the library refuses one that is not above 0)
      tracer.setGISeed(seed);
      crt_bake_stats bs{};
      tracer.bakeLightmap(outPath, b, options, nullptr, &bs);
      std::printf("{\"texels\": %llu, \"covered\": %llu, \"dilated\": %llu, \"raster_ms\": %.4f, \"shoot_ms\": %.4f, \"total_ms\": %.4f}\n",
                  (unsigned long long)bs.texels, (unsigned long long)bs.covered, (unsigned long long)bs.dilated, bs.raster_ms, bs.shoot_ms, bs.total_ms);
      return 0;
    }
    if (probes) {
      // the irradiance probe volume: with --gi N 1, N GI samples per hit under the keys of --seed
      if (probeRays != -1) volume.rays = (uint32_t)probeRays;   // (the library refuses a count outside 1 .. 4096)
      volume.gi_seed = seed;
      crt_probe_stats ps{};
      crt_probe_visibility visibility{};
      std::vector<crt_probe_depth> depth;
      if (probeVisibility) {
        if (crt_probe_visibility_defaults(&volume, &visibility) != CRT_OK) {
          std::fprintf(stderr, "error: --probe-visibility: the probe volume is not valid\n");
          return 1;
        }
        if (probeMaxDistanceGiven) {   // (the library refuses a distance that is not finite and > 0)
          visibility.max_distance = probeMaxDistance;
          visibility.variance_floor = 1e-6f * (probeMaxDistance * probeMaxDistance);
        }
      }
      // --probe-lit: the volume holds what a hit's sample rays would return, the radiance one bounce short of the frame's depth
      crt::RenderOptions bakeOptions(options);
      if (probeLit && bakeOptions.MAX_DEPTH > 0) bakeOptions.MAX_DEPTH--;
      const std::vector<crt_probe> records = probeVisibility ? tracer.bakeProbesVisible(volume, visibility, bakeOptions, &depth, &ps) : tracer.bakeProbes(volume, bakeOptions, &ps);
      if (!probeDepthOut.empty()) {
        FILE *f = std::fopen(probeDepthOut.c_str(), "wb");
        if (!f || std::fwrite(depth.data(), sizeof(crt_probe_depth), depth.size(), f) != depth.size()) {
          std::fprintf(stderr, "error: cannot write %s\n", probeDepthOut.c_str());
          return 1;
        }
        std::fclose(f);
      }
      if (!probesOut.empty()) {
        FILE *f = std::fopen(probesOut.c_str(), "wb");
        if (!f || std::fwrite(records.data(), sizeof(crt_probe), records.size(), f) != records.size()) {
          std::fprintf(stderr, "error: cannot write %s\n", probesOut.c_str());
          return 1;
        }
        std::fclose(f);
      }
      crt_probe_lit_stats ls{};
      if (probeLit) {
        crt::RenderOptions litOptions(options);
        if (probeLitSamples >= 0) litOptions.GI_SAMPLE_SIZE = (unsigned)probeLitSamples;
        tracer.renderProbeLit(outPath, litOptions, volume, records, probeVisibility ? &visibility : nullptr, probeVisibility ? &depth : nullptr, &ls);
      }
      else if (probeVisibility) tracer.probeIrradianceView(outPath, volume, records, &visibility, &depth);
      else tracer.probeIrradianceView(outPath, volume, records);
      if (probeLit)
        std::printf("{\"probes\": %llu, \"invalid\": %llu, \"rays\": %llu, \"shoot_ms\": %.4f, \"project_ms\": %.4f, \"total_ms\": %.4f, \"lit\": %llu, \"unlit\": %llu}\n",
                    (unsigned long long)ps.probes, (unsigned long long)ps.invalid, (unsigned long long)ps.rays, ps.shoot_ms, ps.project_ms, ps.total_ms,
                    (unsigned long long)ls.lit, (unsigned long long)ls.unlit);
      else
      std::printf("{\"probes\": %llu, \"invalid\": %llu, \"rays\": %llu, \"shoot_ms\": %.4f, \"project_ms\": %.4f, \"total_ms\": %.4f}\n",
                  (unsigned long long)ps.probes, (unsigned long long)ps.invalid, (unsigned long long)ps.rays, ps.shoot_ms, ps.project_ms, ps.total_ms);
      return 0;
    }
    if (guideBounces > 0) tracer.setGuideBounces((unsigned)guideBounces);
    if (varianceEstimate) {
      crt_variance_estimate e;
      crt_variance_estimate_defaults(&e);
      if (minHistory >= 0.0f) e.min_history = minHistory;
      tracer.setVarianceEstimate(&e);
    }
    tracer.setGISeed(seed);  // frame r of this run uses seed + r (the reference's GI frames all differ: clock() ^ thread id)
    double best = 1e30;
    for (int r = 0; r < repeat; r++) {
      auto a = std::chrono::high_resolution_clock::now();
      if (adaptive) {
        crt_adaptive a;
        crt_adaptive_defaults(&a);
        a.threshold = adaptiveThreshold; a.min_samples = adaptiveMin; a.max_samples = adaptiveMax;
        std::vector<uint32_t> counts;
        tracer.renderAdaptive(r + 1 == repeat && !denoise ? outPath : std::string(), options, a, 1, &counts, split);
        if (denoise) {  // the PPM is the denoised frame; the frame itself stays what it was
          crt_denoise d;
          crt_denoise_defaults(&d);
          if (denoiseIterations >= 0) d.iterations = (uint32_t)denoiseIterations;
          tracer.renderDenoised(r + 1 == repeat ? outPath : std::string(), d, split);
        }
        if (r + 1 == repeat && !countsPath.empty()) {
          const unsigned W = scene.sceneSettings.image.width, H = scene.sceneSettings.image.height;
          FILE *f = std::fopen(countsPath.c_str(), "w");
          if (!f) throw std::runtime_error("cannot write " + countsPath);
          std::fprintf(f, "P2\n%u %u\n%u\n", W, H, std::max(adaptiveMax, 1u));
          for (unsigned y = 0; y < H; y++)
            for (unsigned x = 0; x < W; x++) std::fprintf(f, "%u%c", counts[(size_t)y * W + x], x + 1 == W ? '\n' : ' ');
          std::fclose(f);
        }
      }
      else if (progressive) tracer.renderProgressive(r + 1 == repeat ? outPath : std::string(), options, progressive);
      else tracer.render(r + 1 == repeat ? outPath : std::string(), options);
      auto b = std::chrono::high_resolution_clock::now();
      best = std::min(best, std::chrono::duration<double>(b - a).count());
    }
    if (!tracer.renderNote().empty()) std::fprintf(stderr, "note: %s\n", tracer.renderNote().c_str());
    crt_stats st = tracer.stats();
    // the reference prints the elapsed seconds of the render window (MEASURE_TIME, RayTracer.cpp:289-293)
    std::printf("%.6fs\n", best);
    std::printf("{\"build_s\": %.6f, \"render_s\": %.6f, \"kernel_ms\": %.4f, \"width\": %u, \"height\": %u}\n",
                std::chrono::duration<double>(t1 - t0).count(), best, st.kernel_ms, scene.sceneSettings.image.width,
                scene.sceneSettings.image.height);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
