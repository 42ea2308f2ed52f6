// TEST INFRASTRUCTURE -- not part of the product, never shipped, never on the product path.
//
// Driver for the REAL reference, compiled where its sources lie under /root/reference by
// oracle/Makefile into oracle/_ref/ (git-ignored).  It replaces only what cannot be built in this
// image: the reference's app/main.cpp hard-codes /home/daniel paths (app/main.cpp:12,16) and its
// SceneParser needs RapidJSON, which the image lacks (cmake/FindRapidJSON.cmake:3-17 fetches it
// from the network).  The reference's Scene/Mesh/Material/Light/Camera/Texture types are all
// publicly constructible (Scene.h:50-69, Material.h:15-24, Texture.h:24-58), so this file fills a
// `Scene` from a CRTS blob (oracle/scene_blob.h) and calls the reference's own
// `RayTracer::render` (RayTracer.cpp:204-298).  Nothing of the hot path is restated here.
//
// usage: ref_render <scene.crts> <out.f32> [--depth N] [--mode NAME] [--ppm out.ppm] [--repeat K] [--gi SAMPLES RAYS_PER_PIXEL] [--all-frames]
//   out.f32 = H*W*3 little-endian float32, row 0 = top  (the reference's colorBuffer)
//   prints one JSON line: {"render_s": ..., "build_s": ..., "width": W, "height": H, ...}
// usage: ref_render --camera-ops <ops.txt> <out.txt>
//   drives the reference's own Camera (Camera.cpp:33-70).  ops.txt: first line = position (3) and row-major matrix (9)
//   as hexadecimal float bit patterns; every further line = "<truck|pan|tilt|roll> <3 bit patterns>", applied one after the
//   other to the same camera.  out.txt: the 12 bit patterns of the camera after every operation, one line each.
// usage: ref_render --rays <scene.crts> <rays.bin> <out.bin> --what trace|occluded|shoot|camera --type T [--depth N] [--gi-occlusion]
//                    [--gi N --seeds <seeds.bin> [--monte-carlo-bias X] [--centre]]
//   answers single rays with the reference's own functions on the scene of the blob; T = 0..4, the value of enum RayType (Ray.h:14).
//   T and N may be comma-separated lists: the trees are built once and out.bin holds one block of records per type (and, for shoot,
//   per type and depth, the depth running fastest), each block in ray order.
//   rays.bin: little-endian float32, 6 per ray (origin xyz, direction xyz; the direction is handed over as given), followed, for
//   `occluded`, by one float32 distance per ray (all rays first, then all distances).  out.bin, one fixed-size record per ray:
//     trace     48 bytes: float32 t, point[3], normal[3], u, v; uint32 mesh, triangle, hit -- what
//               AccelerationStructure(scene).intersect(Ray(o, d, T)) returns (KDTree.cpp:127-192).  mesh = index into scene.objects and
//               triangle = index into that mesh's `triangles`, both from the returned pointers; u, v only in the USE_TEXTURES build
//               (the other build's IntersectionInformation has no such members, Scene.h:44-47: 0 there); no hit: 48 zero bytes.
//     occluded  1 byte: checkForIntersection(Ray(o, d, T), distance, useGI) (AccelerationStructure.cpp:56-94), useGI = --gi-occlusion.
//     shoot     12 bytes: float32 r, g, b of RayTracer::shootRay(ray, 0) (RayTracer.cpp:419-451) on a RayTracer whose renderOptions,
//               useBounding and boundingType are what render() leaves behind for the default tree mode with MAX_DEPTH = N
//               (RayTracer.cpp:205, 270-273).  shootRay and those members are private (RayTracer.h:60-94): this translation unit
//               alone includes that header with `private` spelt `public`, after every standard header; access is no part of a
//               mangled name, so it links against the reference's unmodified objects.
//   --gi N --seeds seeds.bin [--monte-carlo-bias X]  (shoot, camera): the GI build's renderOptions -- USE_GI, GI_SAMPLE_SIZE = N, RAYS_PER_PIXEL
//               = 1, MONTE_CARLO_BIAS = X (default 1e-4) -- and, before every ray, RayTracer::engine.seed(seeds[i]) on this (the main) thread
//               (seeds.bin: one little-endian uint32 per ray).  The engine is the reference's own thread_local member
//               (RayTracer.cpp:28-29); seeding it replaces clock() ^ thread id and nothing else, so the draws of shootRay and getRay
//               are the reference's distribution(engine) on a known stream.
//     camera    rays.bin: uint32 (row, col) per entry.  24 bytes: the Ray getRay(row, col, true) returns under the entry's seed
//               (RayTracer.cpp:61-80).  With --centre, 36 bytes: getRay(row, col, false), then -- the engine seeded -- shootRay(that ray, 0).
// usage: ref_render --gi-draws FIRST COUNT <out.bin>
//   for every seed in [FIRST, FIRST + COUNT): RayTracer::engine.seed(seed), then RayTracer::distribution(RayTracer::engine) twice;
//   out.bin: the two float32 bit patterns per seed.
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <limits>
#include <mutex>
#include <optional>
#include <ostream>
#include <queue>
#include <random>
#include <stack>
#include <string>
#include <thread>
#include <vector>

#define private public   // for RayTracer::shootRay (see --rays above); every standard header is already in
#include "tracer/RayTracer.h"
#undef private
#include "tracer/Scene.h"

#include "scene_blob.h"

static RenderOptimization parseMode(const std::string &s) {
  if (s == "none") return NoOptimization;
  if (s == "regions") return Regions;
  if (s == "pool") return BucketsThreadPool;
  if (s == "queue") return BucketsQueue;
  if (s == "aabb") return AABB;
  if (s == "aabbpool") return BucketsThreadPoolAABB;
  if (s == "aabbqueue") return BucketsQueueAABB;
  if (s == "bvh") return BVH;
  if (s == "bvhpool") return BVHBucketsThreadPool;
  if (s == "bvhqueue") return BVHBucketsQueue;
  std::fprintf(stderr, "unknown mode %s\n", s.c_str());
  std::exit(2);
}

static float bitsToFloat(const std::string &hex) {
  const uint32_t u = (uint32_t)std::strtoul(hex.c_str(), nullptr, 16);
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

static int cameraOps(const char *opsPath, const char *outPath) {
  std::ifstream in(opsPath);
  std::ofstream out(outPath);
  std::string tok;
  float v[12];
  for (int i = 0; i < 12; i++) {
    if (!(in >> tok)) return 2;
    v[i] = bitsToFloat(tok);
  }
  Camera camera(Vector(v[0], v[1], v[2]));
  camera.setRotationMatrix() = Matrix<3>(std::vector<float>(v + 3, v + 12));
  std::string op;
  while (in >> op) {
    float a[3];
    for (int i = 0; i < 3; i++) {
      if (!(in >> tok)) return 2;
      a[i] = bitsToFloat(tok);
    }
    if (op == "truck") camera.truck(Vector(a[0], a[1], a[2]));
    else if (op == "pan") camera.pan(a[0]);
    else if (op == "tilt") camera.tilt(a[0]);
    else if (op == "roll") camera.roll(a[0]);
    else return 2;
    float r[12] = {camera.getPosition()[0], camera.getPosition()[1], camera.getPosition()[2]};
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) r[3 + 3 * i + j] = camera.getRotationMatrix()[i][j];
    char line[160];
    int n = 0;
    for (int i = 0; i < 12; i++) {
      uint32_t u;
      std::memcpy(&u, &r[i], 4);
      n += std::snprintf(line + n, sizeof(line) - n, "%08x%c", u, i == 11 ? '\n' : ' ');
    }
    out << line;
  }
  return 0;
}

struct TexRec { uint32_t kind; float a[3], b[3], s; uint32_t w, h; std::string file; };

// fills `scene` from the CRTS blob at blobPath; bitmaps go through files named after outPath (removed by the caller)
static int loadScene(const std::string &blobPath, const std::string &outPath, Scene &scene, std::vector<TexRec> &texRecs) {
  std::ifstream in(blobPath, std::ios::binary);
  std::vector<char> data((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  blob_cursor c;
  blob_init(&c, data.data(), data.size());
  const void *magic = blob_take(&c, 4);
  if (!magic || std::memcmp(magic, "CRTS", 4) != 0 || blob_u32(&c) != 1) {
    std::fprintf(stderr, "bad blob\n");
    return 2;
  }

  scene.sceneSettings.image.width = blob_u32(&c);
  scene.sceneSettings.image.height = blob_u32(&c);
  scene.sceneSettings.bucketSize = blob_u32(&c);
  float f[9];
  blob_f32v(&c, f, 3);
  scene.sceneSettings.sceneBackgroundColor = Color(f[0], f[1], f[2]);
  blob_f32v(&c, f, 3);
  scene.camera.setPosition() = Vector(f[0], f[1], f[2]);
  blob_f32v(&c, f, 9);
  scene.camera.setRotationMatrix() = Matrix<3>(std::vector<float>(f, f + 9));

  // ---- textures
  uint32_t nTex = blob_u32(&c);
  for (uint32_t t = 0; t < nTex; t++) {
    TexRec r;
    r.kind = blob_u32(&c);
    blob_f32v(&c, r.a, 3);
    blob_f32v(&c, r.b, 3);
    r.s = blob_f32(&c);
    r.w = blob_u32(&c);
    r.h = blob_u32(&c);
    if (r.kind == 3) {
      const void *px = blob_take(&c, (size_t)r.w * r.h * 3);
      r.file = outPath + ".tex" + std::to_string(t) + ".ppm";  // decoded by the reference's own stb_image
      std::ofstream o(r.file, std::ios::binary);
      o << "P6\n" << r.w << " " << r.h << "\n255\n";
      o.write((const char *)px, (std::streamsize)r.w * r.h * 3);
    }
    texRecs.push_back(r);
  }
#if (defined USE_TEXTURES) && USE_TEXTURES
  for (uint32_t t = 0; t < nTex; t++) {
    const TexRec &r = texRecs[t];
    std::string name = "tex" + std::to_string(t);
    Color a(r.a[0], r.a[1], r.a[2]), b(r.b[0], r.b[1], r.b[2]);
    if (r.kind == 0) scene.textures.push_back(new AlbedoTexture(name, a));
    else if (r.kind == 1) scene.textures.push_back(new EdgeTexture(name, a, b, r.s));
    else if (r.kind == 2) scene.textures.push_back(new CheckerTexture(name, a, b, r.s));
    else scene.textures.push_back(new BitmapTexture(name, r.file));
  }
#else
  if (nTex != 0) {
    std::fprintf(stderr, "scene has textures: use the USE_TEXTURES build (ref_render_tex)\n");
    return 2;
  }
#endif

  // ---- materials (reserve first: Mesh keeps `const Material&`, Scene.h:27)
  uint32_t nMat = blob_u32(&c);
  scene.materials.reserve(nMat);
  for (uint32_t m = 0; m < nMat; m++) {
    uint32_t type = blob_u32(&c);
    blob_f32v(&c, f, 3);
    uint32_t smooth = blob_u32(&c);
    float ior = blob_f32(&c);
    int32_t tex = blob_i32(&c);
    Albedo albedo(f[0], f[1], f[2]);
#if (defined USE_TEXTURES) && USE_TEXTURES
    const Texture *texture;
    if (tex >= 0) {
      texture = scene.textures[tex];
    } else {  // constant albedo expressed the way the textured build does it (Texture.cpp:14-16)
      scene.textures.push_back(new AlbedoTexture("albedo" + std::to_string(m), albedo));
      texture = scene.textures.back();
    }
    scene.materials.push_back(Material(*texture, albedo, (MaterialType)type, smooth != 0, ior));
#else
    (void)tex;
    scene.materials.push_back(Material(albedo, (MaterialType)type, smooth != 0, ior));
#endif
  }

  uint32_t nLights = blob_u32(&c);
  for (uint32_t l = 0; l < nLights; l++) {
    blob_f32v(&c, f, 3);
    uint32_t intensity = blob_u32(&c);
    scene.lights.push_back(Light{Vector(f[0], f[1], f[2]), intensity});
  }

  // ---- meshes (reserve + rvalue push_back: triangles point into their own mesh's vertices, Triangle.h:10)
  uint32_t nMesh = blob_u32(&c);
  scene.objects.reserve(nMesh);
  for (uint32_t m = 0; m < nMesh; m++) {
    uint32_t mat = blob_u32(&c), nv = blob_u32(&c), nt = blob_u32(&c), hasUV = blob_u32(&c);
    const float *pos = (const float *)blob_take(&c, (size_t)nv * 12);
    const float *uvs = hasUV ? (const float *)blob_take(&c, (size_t)nv * 12) : nullptr;
    const uint32_t *idx = (const uint32_t *)blob_take(&c, (size_t)nt * 12);
    if (!c.ok) break;
    std::vector<Vertex> vertices;
    vertices.reserve(nv);
    for (uint32_t v = 0; v < nv; v++) {
      vertices.push_back(Vertex(Vector(pos[3 * v], pos[3 * v + 1], pos[3 * v + 2])));
#if (defined USE_TEXTURES) && USE_TEXTURES
      if (uvs) vertices.back().UV = Vector(uvs[3 * v], uvs[3 * v + 1], uvs[3 * v + 2]);
#endif
    }
    (void)uvs;
    std::vector<unsigned int> triples(idx, idx + (size_t)nt * 3);
    scene.objects.push_back(Mesh{scene.materials[mat], vertices, triples});
  }
  if (!c.ok) {
    std::fprintf(stderr, "truncated blob\n");
    return 2;
  }

  return 0;
}

static void removeBitmaps(const std::vector<TexRec> &texRecs) {
  for (auto &r : texRecs)
    if (!r.file.empty()) std::remove(r.file.c_str());
}

struct HitRecord { float t, point[3], normal[3], u, v; uint32_t mesh, triangle, hit; };
static_assert(sizeof(HitRecord) == 48, "HitRecord");

static int giDraws(const char *first, const char *count, const char *outPath) {
  const unsigned long long f = std::strtoull(first, nullptr, 0), n = std::strtoull(count, nullptr, 0);
  std::vector<float> draws(2 * (size_t)n);
  for (unsigned long long i = 0; i < n; i++) {
    RayTracer::engine.seed((unsigned long)(f + i));
    draws[2 * i] = RayTracer::distribution(RayTracer::engine);
    draws[2 * i + 1] = RayTracer::distribution(RayTracer::engine);
  }
  std::ofstream out(outPath, std::ios::binary);
  out.write((const char *)draws.data(), (std::streamsize)draws.size() * 4);
  out.close();
  std::printf("\n{\"first\": %llu, \"count\": %llu}\n", f, n);
  return out.good() ? 0 : 2;
}

static int rayQueries(int argc, char **argv) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: %s --rays scene.crts rays.bin out.bin --what trace|occluded|shoot --type T [--depth N] [--gi-occlusion]\n", argv[0]);
    return 2;
  }
  std::string blobPath = argv[2], raysPath = argv[3], outPath = argv[4], what;
  std::vector<int> types;
  std::vector<unsigned> depths;
  bool giOcclusion = false, useGI = false, centre = false;
  unsigned giSamples = 0;
  float monteCarloBias = 1e-4;
  std::string seedsPath;
  auto numbers = [](const std::string &list) {   // "2" or "0,1,2,3"
    std::vector<int> v;
    for (size_t at = 0; at <= list.size();) {
      size_t comma = std::min(list.find(',', at), list.size());
      v.push_back(std::atoi(list.substr(at, comma - at).c_str()));
      at = comma + 1;
    }
    return v;
  };
  for (int i = 5; i < argc; i++) {
    std::string a = argv[i];
    if (a == "--what" && i + 1 < argc) what = argv[++i];
    else if (a == "--type" && i + 1 < argc) types = numbers(argv[++i]);
    else if (a == "--depth" && i + 1 < argc) { for (int d : numbers(argv[++i])) depths.push_back((unsigned)d); }
    else if (a == "--gi-occlusion") giOcclusion = true;
    else if (a == "--gi" && i + 1 < argc) { useGI = true; giSamples = (unsigned)std::atoi(argv[++i]); }
    else if (a == "--seeds" && i + 1 < argc) seedsPath = argv[++i];
    else if (a == "--monte-carlo-bias" && i + 1 < argc) monteCarloBias = std::strtof(argv[++i], nullptr);
    else if (a == "--centre") centre = true;
    else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); return 2; }
  }
  if (depths.empty()) depths.push_back(5);
  bool typesOk = !types.empty();
  for (int t : types) typesOk = typesOk && t >= (int)PrimaryRay && t <= (int)DiffuseRay;
  if (what == "camera" && types.empty()) { types.push_back((int)PrimaryRay); typesOk = true; }
  if ((what != "trace" && what != "occluded" && what != "shoot" && what != "camera") || !typesOk) {
    std::fprintf(stderr, "--what trace|occluded|shoot|camera and --type 0..4 are required\n");
    return 2;
  }
  if (useGI != !seedsPath.empty() || (useGI && what != "shoot" && what != "camera") || (what == "camera" && !useGI)) {
    std::fprintf(stderr, "--gi N and --seeds FILE go together, with --what shoot or camera; camera needs them\n");
    return 2;
  }

  std::ifstream in(raysPath, std::ios::binary);
  std::vector<char> bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  const size_t perRay = what == "occluded" ? 28 : what == "camera" ? 8 : 24;
  if (!in.good() && !in.eof()) return 2;
  if (bytes.size() % perRay != 0) {
    std::fprintf(stderr, "%s: %zu bytes is no multiple of %zu\n", raysPath.c_str(), bytes.size(), perRay);
    return 2;
  }
  const size_t n = bytes.size() / perRay;
  std::vector<float> values(bytes.size() / 4);
  std::memcpy(values.data(), bytes.data(), bytes.size());
  const float *rays = values.data(), *distances = values.data() + 6 * n;
  std::vector<uint32_t> seeds;
  if (useGI) {
    std::ifstream sin(seedsPath, std::ios::binary);
    std::vector<char> sb((std::istreambuf_iterator<char>(sin)), std::istreambuf_iterator<char>());
    if (sb.size() != 4 * n) {
      std::fprintf(stderr, "%s: %zu bytes, expected one uint32 for each of %zu rays\n", seedsPath.c_str(), sb.size(), n);
      return 2;
    }
    seeds.resize(n);
    std::memcpy(seeds.data(), sb.data(), sb.size());
  }

  Scene scene;
  std::vector<TexRec> texRecs;
  if (int rc = loadScene(blobPath, outPath, scene, texRecs)) return rc;

  std::ofstream out(outPath, std::ios::binary);
  auto rayOf = [&](size_t i, int type) {
    const RayType rayType = (RayType)type;
    return Ray(Vector(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]), Vector(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]), rayType);
  };
  if (what == "shoot") {
    RayTracer tracer(scene);
    // the state render() leaves behind for the default tree mode (RayTracer.cpp:205, 270-273), set directly: no frame is wanted
    tracer.useBounding = true;
    tracer.boundingType = Tree;
    std::vector<float> rgb(3 * n);
    for (int type : types)
      for (unsigned depth : depths) {
        tracer.renderOptions = useGI ? RenderOptions(BVHBucketsThreadPool, depth, true, giSamples, 1, 1e-4, 1e-4, 1e-4, monteCarloBias)
                                     : RenderOptions(BVHBucketsThreadPool, depth);
        for (size_t i = 0; i < n; i++) {
          Ray ray = rayOf(i, type);
          if (useGI) RayTracer::engine.seed(seeds[i]);
          Color c = tracer.shootRay(ray, 0);
          for (int k = 0; k < 3; k++) rgb[3 * i + k] = c[k];
        }
        out.write((const char *)rgb.data(), (std::streamsize)rgb.size() * 4);
      }
  } else if (what == "camera") {
    RayTracer tracer(scene);
    tracer.useBounding = true;
    tracer.boundingType = Tree;
    tracer.renderOptions = RenderOptions(BVHBucketsThreadPool, depths[0], true, giSamples, 1, 1e-4, 1e-4, 1e-4, monteCarloBias);
    std::vector<uint32_t> pixels(2 * n);
    std::memcpy(pixels.data(), bytes.data(), bytes.size());
    for (size_t i = 0; i < n; i++) {
      float rec[9];
      RayTracer::engine.seed(seeds[i]);
      Ray ray = tracer.getRay(pixels[2 * i], pixels[2 * i + 1], !centre);
      for (int k = 0; k < 3; k++) { rec[k] = ray.origin[k]; rec[3 + k] = ray.direction[k]; }
      if (centre) {
        RayTracer::engine.seed(seeds[i]);
        Color c = tracer.shootRay(ray, 0);
        for (int k = 0; k < 3; k++) rec[6 + k] = c[k];
      }
      out.write((const char *)rec, centre ? 36 : 24);
    }
  } else {
    AccelerationStructure accel(scene);
    for (int type : types) {
      if (what == "occluded") {
        std::vector<uint8_t> occ(n);
        for (size_t i = 0; i < n; i++) occ[i] = accel.checkForIntersection(rayOf(i, type), distances[i], giOcclusion) ? 1 : 0;
        out.write((const char *)occ.data(), (std::streamsize)n);
      } else {
        std::vector<HitRecord> recs(n);
        std::memset(recs.data(), 0, n * sizeof(HitRecord));
        for (size_t i = 0; i < n; i++) {
          std::optional<IntersectionInformation> info = accel.intersect(rayOf(i, type));
          if (!info.has_value()) continue;
          HitRecord &r = recs[i];
          r.t = info->intersection.distance;
          for (int k = 0; k < 3; k++) {
            r.point[k] = info->intersection.hitPoint[k];
            r.normal[k] = info->intersection.hitNormal[k];
          }
#if (defined USE_TEXTURES) && USE_TEXTURES
          r.u = info->u;
          r.v = info->v;
#endif
          r.mesh = (uint32_t)(info->object - scene.objects.data());
          r.triangle = (uint32_t)(info->triangle - info->object->triangles.data());
          r.hit = 1;
        }
        out.write((const char *)recs.data(), (std::streamsize)(n * sizeof(HitRecord)));
      }
    }
  }
  out.close();
  removeBitmaps(texRecs);
  std::printf("\n{\"rays\": %zu, \"what\": \"%s\", \"types\": %zu, \"depths\": %zu}\n", n, what.c_str(), types.size(), depths.size());
  return out.good() ? 0 : 2;
}

int main(int argc, char **argv) {
  if (argc == 4 && std::string(argv[1]) == "--camera-ops") return cameraOps(argv[2], argv[3]);
  if (argc >= 2 && std::string(argv[1]) == "--rays") return rayQueries(argc, argv);
  if (argc == 5 && std::string(argv[1]) == "--gi-draws") return giDraws(argv[2], argv[3], argv[4]);
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s scene.crts out.f32 [--depth N] [--mode NAME] [--ppm P] [--repeat K] [--gi SAMPLES RAYS_PER_PIXEL] [--all-frames]\n", argv[0]);
    return 2;
  }
  std::string blobPath = argv[1], outPath = argv[2], ppmPath, mode = "bvhpool";
  unsigned depth = 5;
  int repeat = 1;
  bool useGI = false, allFrames = false;
  unsigned giSamples = 2, raysPerPixel = 1;
  for (int i = 3; i < argc; i++) {
    std::string a = argv[i];
    if (a == "--depth" && i + 1 < argc) depth = std::atoi(argv[++i]);
    else if (a == "--mode" && i + 1 < argc) mode = argv[++i];
    else if (a == "--ppm" && i + 1 < argc) ppmPath = argv[++i];
    else if (a == "--repeat" && i + 1 < argc) repeat = std::atoi(argv[++i]);
    else if (a == "--gi" && i + 2 < argc) { useGI = true; giSamples = (unsigned)std::atoi(argv[++i]); raysPerPixel = (unsigned)std::atoi(argv[++i]); }
    else if (a == "--all-frames") allFrames = true;
  }

  Scene scene;
  std::vector<TexRec> texRecs;
  if (int rc = loadScene(blobPath, outPath, scene, texRecs)) return rc;

  const unsigned W = scene.sceneSettings.image.width, H = scene.sceneSettings.image.height;
  auto t0 = std::chrono::high_resolution_clock::now();
  RayTracer tracer(scene);
  auto t1 = std::chrono::high_resolution_clock::now();
  // --gi N R: the GI / multi-sample mode (RayTracer.h:27-30) -- every render then differs (the reference seeds its generator
  // from clock() ^ thread id), so --all-frames writes each of the --repeat frames, for statistics over them
  RenderOptions options(parseMode(mode), depth, useGI, giSamples, raysPerPixel);
  std::vector<std::vector<Color>> buffer;
  double best = 1e30, total = 0;
  std::ofstream out(outPath, std::ios::binary);
  std::vector<float> flat((size_t)W * H * 3);
  for (int r = 0; r < repeat; r++) {
    auto a = std::chrono::high_resolution_clock::now();
    buffer = tracer.render(r == repeat - 1 ? ppmPath : std::string(), options);
    auto b = std::chrono::high_resolution_clock::now();
    double s = std::chrono::duration<double>(b - a).count();
    total += s;
    if (s < best) best = s;
    if (allFrames || r == repeat - 1) {
      for (unsigned y = 0; y < H; y++)
        for (unsigned x = 0; x < W; x++)
          for (unsigned k = 0; k < 3; k++) flat[((size_t)y * W + x) * 3 + k] = buffer[y][x][k];
      out.write((const char *)flat.data(), (std::streamsize)flat.size() * 4);
    }
  }
  removeBitmaps(texRecs);

  std::printf("\n{\"render_s\": %.6f, \"render_s_mean\": %.6f, \"build_s\": %.6f, \"width\": %u, \"height\": %u, "
              "\"depth\": %u, \"mode\": \"%s\", \"threads\": %u, \"repeat\": %d}\n",
              best, total / repeat, std::chrono::duration<double>(t1 - t0).count(), W, H, depth, mode.c_str(),
              std::thread::hardware_concurrency(), repeat);
  return 0;
}
