"""Dev helper (GPU box): what the variance estimate costs.  HW14, full detail, at 960x540 and 1920x1080, max_depth 3, gi_sample_size 2, warm
context, HIP events, median of --repeats after --warmup calls, one session:
  (a) crt_variance_estimate_device on records that crt_temporal_device wrote, under the first hits of the camera's rays, in three
      conditions: every pixel flagged (one sample, no history), no pixel flagged (eight samples: the skip route of every tile), and a panned
      camera (the history of eight samples reprojected: only the disoccluded pixels are flagged).  Beside it a device-to-device copy of
      the bytes the call must move: 64 (a record's line) + 48 (a crt_hit) + 4 read and 4 written, 120 a pixel: a copy of 60 bytes a pixel
  (b) the four post-processing frame calls on a one-sample frame with the setting off and on, without host copies
  (c) with --frame-roots PARENT,THIS: (b)'s calls with the setting off in a fresh process of each checkout's own library, alternating,
      --frame-runs times
  (d) with --bench-roots PARENT,THIS: `bench.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline` of each root, alternating, --bench-runs
      times (no frame code object changed: the ranges should overlap)
usage: python tools/variance_time.py --out profiles/variance_estimate.json [--frame-roots PARENT,.] [--bench-roots PARENT,.]"""
import argparse, importlib, json, os, subprocess, sys
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--sizes", default="960x540,1920x1080")
ap.add_argument("--out", default="")
ap.add_argument("--commit", default="", help="recorded with the numbers (default: git rev-parse HEAD in --root, if that works)")
ap.add_argument("--frames-only", action="store_true", help="(b) alone, for --root's own library: what --frame-roots runs")
ap.add_argument("--frame-roots", default="", help="two checkouts, comma-separated: the parent's and this tree's")
ap.add_argument("--frame-runs", type=int, default=2)
ap.add_argument("--bench-roots", default="", help="two checkouts, comma-separated: the parent's and this tree's")
ap.add_argument("--bench-runs", type=int, default=3)
args = ap.parse_args()
sys.path.insert(0, args.root)
import torch
pkg = importlib.import_module("course-assignment-danielhalachev_amd"); sc = pkg.scenes
DEPTH, SAMPLES, SEED = 3, 2, 7
PAN_DEGREES, SHIFT = 8.0, (0.25, 0.05, 0.1)   # the move of tests/test_gpu_temporal.py


def commit():
    if args.commit:
        return args.commit
    try:
        return subprocess.check_output(["git", "-C", args.root, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        return "unknown"


torch.zeros(1, device="cuda")
stream = torch.cuda.current_stream()
one = pkg.make_adaptive(min_samples=1, max_samples=1)   # one sample for every pixel
HAS_SETTING = hasattr(pkg.Tracer, "set_variance_estimate")


def options(seed):
    return pkg.make_options(DEPTH, use_gi=True, gi_sample_size=SAMPLES, rays_per_pixel=1, gi_seed=seed)


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def median_of(call):
    ms = [timed(call) for _ in range(args.warmup + args.repeats)][args.warmup:]
    return {"ms": float(np.median(ms)), "ms_min": float(min(ms))}


def moved(camera):
    a = np.radians(PAN_DEGREES)
    ry = np.array([[np.cos(a), 0, -np.sin(a)], [0, 1, 0], [np.sin(a), 0, np.cos(a)]])
    m = (np.asarray(camera[1], dtype=np.float64).reshape(3, 3) @ ry).astype(np.float32).reshape(9)
    return (np.asarray(camera[0], dtype=np.float32) + np.array(SHIFT, dtype=np.float32)).astype(np.float32), m


def frame_calls(tracer, entry):
    """(b): the four calls on a one-sample frame, second frame of its history, no host copies"""
    L = pkg.lib()
    t, d = pkg.make_temporal(), pkg.make_denoise()
    for split, tag in ((False, ""), (True, "_split")):
        for seed in (SEED, SEED + 1):   # the first frame sizes the context and leaves a history
            tracer.render_adaptive(options(seed), one, split=split)
            tracer.render_accumulated(t, d, split=split)
        den = L.crt_render_denoised_split if split else L.crt_render_denoised
        acc = L.crt_render_accumulated_split if split else L.crt_render_accumulated
        for on in (False, True) if HAS_SETTING else (False,):
            if HAS_SETTING:
                tracer.set_variance_estimate(pkg.make_variance_estimate() if on else None)
            tracer._check(den(tracer.ctx, d, None, None))   # (the setting's scratch records are allocated outside the timing)
            key = "_on" if on else "_off"
            entry["b_render_denoised" + tag + key] = median_of(lambda: tracer._check(den(tracer.ctx, d, None, None)))
            entry["b_render_accumulated" + tag + key] = median_of(lambda: tracer._check(acc(tracer.ctx, t, d, None, None, None)))
        if HAS_SETTING:
            tracer.set_variance_estimate(None)


def measure(width, height):
    hs = pkg.Scene(json_text=sc.to_json(sc.make("hw14", width=width, height=height)))
    tracer = pkg.Tracer(hs)
    n = width * height
    entry = {"pixels": n}
    frame_calls(tracer, entry)
    if args.frames_only:
        tracer.close()
        return entry
    own = hs.camera()
    t, e = pkg.make_temporal(), pkg.make_variance_estimate()
    rng = np.random.default_rng(3)

    def state(samples):
        colours = rng.random((samples, n, 3), dtype=np.float32)
        return (torch.from_numpy(colours.sum(axis=0)).cuda(), torch.from_numpy((colours * colours).sum(axis=(0, 2))).cuda(),
                torch.full((n,), samples, dtype=torch.int32, device="cuda"))

    def hits_of(camera):
        rays = torch.zeros((n, 6), device="cuda")
        hits = torch.zeros((n, 48), dtype=torch.uint8, device="cuda")
        tracer.set_camera(*camera)
        tracer.camera_rays_device(rays.data_ptr())
        tracer.trace_rays_device(rays.data_ptr(), n, pkg.RAY_PRIMARY, hits.data_ptr())
        torch.cuda.synchronize()
        return hits

    def records_of(st, hits, prev=None, prev_pose=None):
        nxt = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
        rgb, var = torch.zeros((n, 3), device="cuda"), torch.zeros((n,), device="cuda")
        tracer.temporal_device(t, width, height, prev_pose, prev.data_ptr() if prev is not None else None, st[0].data_ptr(), st[1].data_ptr(),
                               st[2].data_ptr(), hits.data_ptr(), nxt.data_ptr(), rgb.data_ptr(), d_out_var_ptr=var.data_ptr())
        torch.cuda.synchronize()
        return nxt, var

    hits_own, hits_moved = hits_of(own), hits_of(moved(own))
    tracer.set_camera(*own)
    long_records, long_var = records_of(state(8), hits_own)
    cases = {"every_pixel_flagged": (records_of(state(1), hits_own), hits_own), "no_pixel_flagged": ((long_records, long_var), hits_own),
             "panned_camera": (records_of(state(1), hits_moved, long_records, pkg.make_pose(*own)), hits_moved)}
    out = torch.zeros((n,), device="cuda")
    for name, ((records, var), hits) in cases.items():
        call = lambda: tracer.variance_estimate_device(e, width, height, records.data_ptr(), hits.data_ptr(), var.data_ptr(), out.data_ptr())
        call()
        torch.cuda.synchronize()
        entry["a_" + name] = median_of(call)
        entry["a_" + name]["share_of_pixels_changed"] = float((out.view(torch.int32) != var.view(torch.int32)).float().mean().item())
    src, dst = torch.zeros((60 * n,), dtype=torch.uint8, device="cuda"), torch.zeros((60 * n,), dtype=torch.uint8, device="cuda")
    entry["a_copy_of_60_bytes_a_pixel"] = median_of(lambda: dst.copy_(src))
    entry["a_bytes_moved"] = 120 * n
    tracer.close()
    return entry


result = {"scene": "hw14 full detail", "max_depth": DEPTH, "gi_sample_size": SAMPLES, "gi_seed": SEED, "samples_per_pixel": 1, "repeats": args.repeats,
          "warmup": args.warmup, "commit": commit(), "csrc_sha256": pkg.csrc_sha256(), "device": torch.cuda.get_device_name(0), "sizes": {}}
for size in args.sizes.split(","):
    w, h = (int(v) for v in size.split("x"))
    result["sizes"][size] = measure(w, h)
    print(size, json.dumps(result["sizes"][size]), flush=True)


def alternate(roots, runs, command, parse):
    """a fresh process of each checkout, alternating: the checkout's own library"""
    got = {r: [] for r in roots}
    for _ in range(runs):
        for r in roots:
            p = subprocess.run(command(r), cwd=r, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit("%r failed: %s" % (command(r), p.stderr[-2000:]))
            got[r].append(parse(p.stdout))
            print(r, got[r][-1], flush=True)
    return {"parent": got[roots[0]], "this_tree": got[roots[1]]}


if args.frame_roots and not args.frames_only:
    roots = [os.path.abspath(r) for r in args.frame_roots.split(",")]
    me = os.path.abspath(__file__)
    result["c_frame_calls_alternating"] = alternate(
        roots, args.frame_runs, lambda r: [sys.executable, me, "--root", r, "--frames-only", "--commit", "-", "--sizes", args.sizes],
        lambda text: {size: {k: v["ms"] for k, v in e.items() if k.endswith("_off")} for size, e in json.loads(text.strip().splitlines()[-1])["sizes"].items()})
if args.bench_roots and not args.frames_only:
    roots = [os.path.abspath(r) for r in args.bench_roots.split(",")]

    def bench_line(text):
        j = json.loads([ln for ln in text.splitlines() if ln.startswith('{"metric"')][-1])
        return {"value": j["value"], "unit": j.get("unit"), "ms_per_step": j.get("ms_per_step")}
    result["d_bench_alternating"] = alternate(
        roots, args.bench_runs, lambda r: [sys.executable, os.path.join(r, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline"],
        bench_line)
print(json.dumps(result))
if args.out:
    json.dump(result, open(args.out, "w"), indent=1)
