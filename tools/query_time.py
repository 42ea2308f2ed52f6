"""Dev helper (GPU box): what the ray queries cost on the benchmark scene (HW14, full detail, 1920x1080), everything device-resident,
warm context, HIP events on the queries' stream, median of --repeats calls after --warmup:
  (a) trace_rays_device of the frame's own 2,073,600 camera rays (PRIMARY)      (a0) the same with tuning.bvh = 0: the reroute kernel alone
  (b) the same number of random rays in and around the room (incoherent)
  (c) occluded_rays_device from the primary hit points of (a) to the first light
  (d) the device time of a whole max_depth = 0 frame of the same scene and camera (crt_kernel_times_ms phase [0]): it walks the rays of
      (a), shades them, walks their shadow rays and resolves -- a query of the same rays has to be faster.
usage: python tools/query_time.py [--out profiles/query_rays.json]
       python tools/query_time.py --frame-only --root OTHER_CHECKOUT [--out ...]    ((d) alone, with the package of another checkout: it
       uses nothing that a commit without the queries lacks; the results are merged into --out under "frame")"""
import argparse, importlib, json, os, subprocess, sys
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--frame-only", action="store_true")
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default="")
ap.add_argument("--commit", default="", help="recorded with the numbers (default: git rev-parse HEAD in --root, if that works)")
args = ap.parse_args()
sys.path.insert(0, args.root)
import torch
pkg = importlib.import_module("course-assignment-danielhalachev_amd"); sc = pkg.scenes


def commit():
    if args.commit:
        return args.commit
    try:
        return subprocess.check_output(["git", "-C", args.root, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        return "unknown"


scene = sc.make("hw14")
hs = pkg.Scene(json_text=sc.to_json(scene))
W, H = hs.width, hs.height
N = W * H
result = {"scene": "hw14 full detail %dx%d" % (W, H), "repeats": args.repeats, "warmup": args.warmup, "commit": commit(),
          "csrc_sha256": pkg.csrc_sha256(), "device": torch.cuda.get_device_name(0)}


def frame_ms(tracer):
    for _ in range(args.warmup + args.repeats):
        tracer.render(max_depth=0)
    times = [t[0] for t in tracer.kernel_times_ms()[-args.repeats:]]
    assert tracer.stats().fallback_frames == 0
    return float(np.median(times)), float(min(times))


if args.frame_only:
    med, best = frame_ms(pkg.Tracer(hs))
    result.update(depth0_frame_ms=med, depth0_frame_ms_min=best)
    print(json.dumps(result))
    if args.out:
        doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
        doc["frame"] = result
        json.dump(doc, open(args.out, "w"), indent=1)
    sys.exit(0)

stream = torch.cuda.current_stream()


def timed(call, tracer):
    for _ in range(args.warmup):
        call()
    ms = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); call(); e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    st = tracer.query_stats()
    med = float(np.median(ms))
    return {"ms": med, "ms_min": float(min(ms)), "rays": int(st.rays), "hits": int(st.hits), "rerouted": int(st.rerouted),
            "mrays_per_s": st.rays / med / 1e3}


tracer = pkg.Tracer(hs)
d_rays = torch.empty((N, 6), dtype=torch.float32, device="cuda")
d_hits = torch.empty((N, 48), dtype=torch.uint8, device="cuda")
tracer.camera_rays_device(d_rays.data_ptr(), stream.cuda_stream)
result["a_camera_rays_closest"] = timed(lambda: tracer.trace_rays_device(d_rays.data_ptr(), N, pkg.RAY_PRIMARY, d_hits.data_ptr(), stream.cuda_stream), tracer)

# (c) from the hit points of (a) towards the first light, started SHADOW_BIAS off the surface like calculateDiffusion's rays (RayTracer.cpp:308-318)
rec = d_hits.view(torch.float32).reshape(N, 12)
hit = d_hits.view(torch.int32).reshape(N, 12)[:, 11] != 0
point, normal = rec[hit, 1:4], rec[hit, 4:7]
light = torch.tensor(np.asarray(scene["lights"][0]["position"], dtype=np.float32), device="cuda")
origin = point + normal * 1e-4
to_light = light[None, :] - point
dist = torch.linalg.norm(to_light, dim=1)
d_srays = torch.cat([origin, to_light / dist[:, None]], dim=1).contiguous()
d_dist = dist.contiguous()
M = int(d_srays.shape[0])
d_occ = torch.empty(M, dtype=torch.uint8, device="cuda")
result["c_shadow_rays_to_first_light"] = timed(lambda: tracer.occluded_rays_device(d_srays.data_ptr(), d_dist.data_ptr(), M, d_occ.data_ptr(), stream.cuda_stream), tracer)

# (b) tests/query_sets.py: random_rays' recipe, N of them
rng = np.random.default_rng(11)
o = rng.uniform([-3.5, -2.0, -8.5], [3.5, 3.0, 1.5], (N, 3))
d = rng.normal(size=(N, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
d_rand = torch.from_numpy(np.concatenate([o, d], axis=1).astype(np.float32)).cuda()
result["b_random_rays_closest"] = timed(lambda: tracer.trace_rays_device(d_rand.data_ptr(), N, pkg.RAY_REFLECTION, d_hits.data_ptr(), stream.cuda_stream), tracer)

med, best = frame_ms(tracer)
result.update(depth0_frame_ms=med, depth0_frame_ms_min=best)

plain = pkg.Tracer(hs, tuning=pkg.make_tuning(bvh=0))
result["a0_camera_rays_closest_reroute_kernel_alone"] = timed(lambda: plain.trace_rays_device(d_rays.data_ptr(), N, pkg.RAY_PRIMARY, d_hits.data_ptr(), stream.cuda_stream), plain)

for k, v in result.items():
    print(k, v)
print(json.dumps(result))
if args.out:
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    doc["queries"] = result
    json.dump(doc, open(args.out, "w"), indent=1)
