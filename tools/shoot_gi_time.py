"""Dev helper (GPU box): what a radiance query in the GI mode costs beside the GI frame it is a special case of.  HW14, full detail, at
960x540, max_depth 3, gi_sample_size 2, everything device-resident, warm context, HIP events on the query's stream, median of --repeats
calls after --warmup:
  (q) shoot_rays_gi_device of the camera's 518,400 rays as PRIMARY rays with keys=NULL (the keys of a frame's pixels, sample 0): the GI
      frame's pixels through the level-synchronous query (its host waits between the levels are inside the events)
  (f) the device time of a GI frame of the same camera, depth, sample size and seed with rays_per_pixel = 1 (crt_kernel_times_ms [0])
usage: python tools/shoot_gi_time.py [--out profiles/shoot_rays_gi.json]"""
import argparse, importlib, json, os, subprocess, sys
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default="")
ap.add_argument("--commit", default="", help="recorded with the numbers (default: git rev-parse HEAD in --root, if that works)")
args = ap.parse_args()
sys.path.insert(0, args.root)
import torch
pkg = importlib.import_module("course-assignment-danielhalachev_amd"); sc = pkg.scenes
WIDTH, HEIGHT, DEPTH, SAMPLES, SEED = 960, 540, 3, 2, 7


def commit():
    if args.commit:
        return args.commit
    try:
        return subprocess.check_output(["git", "-C", args.root, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        return "unknown"


scene = sc.make("hw14", width=WIDTH, height=HEIGHT)
hs = pkg.Scene(json_text=sc.to_json(scene))
N = hs.width * hs.height
tracer = pkg.Tracer(hs)
options = pkg.make_options(DEPTH, use_gi=True, gi_sample_size=SAMPLES, rays_per_pixel=1, gi_seed=SEED)
result = {"scene": "hw14 full detail %dx%d" % (hs.width, hs.height), "max_depth": DEPTH, "gi_sample_size": SAMPLES, "gi_seed": SEED,
          "repeats": args.repeats, "warmup": args.warmup, "commit": commit(), "csrc_sha256": pkg.csrc_sha256(), "device": torch.cuda.get_device_name(0)}

# (f) the GI frame
frame = None
for _ in range(args.warmup + args.repeats):
    frame = tracer.render(options=options)
times = [t[0] for t in tracer.kernel_times_ms()[-args.repeats:]]
assert tracer.stats().fallback_frames == 0
result["frame_ms"] = float(np.median(times))
result["frame_ms_min"] = float(min(times))

# (q) the query
stream = torch.cuda.current_stream()
d_rays = torch.empty((N, 6), dtype=torch.float32, device="cuda")
d_rgb = torch.empty((N, 3), dtype=torch.float32, device="cuda")
tracer.camera_rays_device(d_rays.data_ptr(), stream.cuda_stream)


def call():
    tracer.shoot_rays_gi_device(d_rays.data_ptr(), N, d_rgb.data_ptr(), None, pkg.RAY_PRIMARY, options, stream_ptr=stream.cuda_stream)


for _ in range(args.warmup):
    call()
ms = []
for _ in range(args.repeats):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream); call(); e1.record(stream)
    e1.synchronize()
    ms.append(e0.elapsed_time(e1))
st = tracer.shoot_stats()
result["query_ms"] = float(np.median(ms))
result["query_ms_min"] = float(min(ms))
result["rays"] = int(st.rays)
result["levels"] = int(st.levels)
result["level_rays"] = [int(x) for x in st.level_rays[:st.levels]]
result["shadow_records"] = int(st.shadow_records)
result["rerouted"] = int(st.rerouted)
result["kernel_ms_last_call"] = float(st.kernel_ms)
result["query_over_frame"] = result["query_ms"] / result["frame_ms"]
# the query's pixels are the frame's (as values: the frame adds its one sample to 0)
got = d_rgb.cpu().numpy().reshape(frame.shape)
result["query_equals_the_frame"] = bool(np.all((got == frame) | (np.isnan(got) & np.isnan(frame))))

for k, v in result.items():
    print(k, v)
print(json.dumps(result))
if args.out:
    json.dump(result, open(args.out, "w"), indent=1)
