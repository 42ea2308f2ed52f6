"""Dev helper (GPU box): what the temporal accumulation costs.  HW14, full detail, at 960x540 and 1920x1080, max_depth 3, gi_sample_size
2, warm context, HIP events, median of --repeats after --warmup calls, one session:
  (a) crt_temporal_device on the frame's own state and first hits, with the previous frame's records (a static camera: every hit pixel has
      its four taps) and without a history; beside it a device-to-device copy of the bytes the call must move at least -- 48 + 12 + 4 + 4
      read of the frame, 64 of the history, 64 + 12 + 4 + 1 written: 213 a pixel, a copy of 107 bytes a pixel
  (b) the whole crt_render_accumulated call at the defaults on the second frame of a context (a history exists), with and without the
      spatial filter, with and without the host copies
  (c) one adaptive pass over the full list, for scale
  (d) with --bench-roots A,B: `bench.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline` of each root, alternating, --bench-runs times (the frame path is not
      touched: the ranges should overlap)
usage: python tools/temporal_time.py --out profiles/temporal.json [--bench-roots PARENT_CHECKOUT,.]"""
import argparse, importlib, json, os, subprocess, sys
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--sizes", default="960x540,1920x1080")
ap.add_argument("--out", default="")
ap.add_argument("--commit", default="", help="recorded with the numbers (default: git rev-parse HEAD in --root, if that works)")
ap.add_argument("--bench-roots", default="", help="two checkouts, comma-separated: the parent's and this tree's")
ap.add_argument("--bench-runs", type=int, default=3)
args = ap.parse_args()
sys.path.insert(0, args.root)
import torch
pkg = importlib.import_module("course-assignment-danielhalachev_amd"); sc = pkg.scenes
DEPTH, SAMPLES, SEED = 3, 2, 7


def commit():
    if args.commit:
        return args.commit
    try:
        return subprocess.check_output(["git", "-C", args.root, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        return "unknown"


torch.zeros(1, device="cuda")
stream = torch.cuda.current_stream()
adaptive = pkg.make_adaptive(min_samples=4, max_samples=4)   # four samples for every pixel
result = {"scene": "hw14 full detail", "max_depth": DEPTH, "gi_sample_size": SAMPLES, "gi_seed": SEED, "samples_per_pixel": 4,
          "repeats": args.repeats, "warmup": args.warmup, "commit": commit(), "csrc_sha256": pkg.csrc_sha256(), "device": torch.cuda.get_device_name(0),
          "sizes": {}}


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


def measure(width, height):
    hs = pkg.Scene(json_text=sc.to_json(sc.make("hw14", width=width, height=height)))
    tracer, L = pkg.Tracer(hs), pkg.lib()
    n = width * height
    entry = {"pixels": n}
    t, d = pkg.make_temporal(), pkg.make_denoise()
    # two frames on one context: the first sizes it and leaves a history, the second is the one measured
    tracer.render_adaptive(options(SEED), adaptive)
    tracer.render_accumulated()
    tracer._check(L.crt_render_adaptive(tracer.ctx, options(SEED + 1), adaptive, 0, 1, None, None))
    passes = [timed(lambda: tracer._check(L.crt_render_adaptive(tracer.ctx, options(SEED + 1), adaptive, s, 1, None, None))) for s in (1, 2, 3)]
    entry["c_adaptive_pass_full_list_ms"] = float(np.median(passes))
    out = np.zeros((height, width, 3), dtype=np.float32)
    taps = np.zeros((height, width), dtype=np.uint8)
    tracer.render_accumulated()      # (traces the guides of this frame)
    call = lambda dn, rgb, valid: tracer._check(L.crt_render_accumulated(tracer.ctx, t, dn, rgb, None, valid))
    entry["b_render_accumulated"] = median_of(lambda: call(None, out.ctypes.data, taps.ctypes.data))
    entry["b_render_accumulated_no_host_copy"] = median_of(lambda: call(None, None, None))
    entry["b_render_accumulated_denoised"] = median_of(lambda: call(d, out.ctypes.data, taps.ctypes.data))
    entry["b_render_accumulated_denoised_no_host_copy"] = median_of(lambda: call(d, None, None))
    entry["b_history_frames"] = tracer.history_frames()
    entry["b_share_of_pixels_with_a_valid_tap"] = float((taps > 0).mean())
    # the primitive on arrays of the caller's: a fold's state of four noisy samples, the first hits of the camera's rays
    rng = np.random.default_rng(3)
    colours = rng.random((4, n, 3), dtype=np.float32)
    total = torch.from_numpy(colours.sum(axis=0)).cuda()
    sq = torch.from_numpy((colours * colours).sum(axis=(0, 2))).cuda()
    counts = torch.full((n,), 4, dtype=torch.int32, device="cuda")
    rays = torch.zeros((n, 6), device="cuda")
    hits = torch.zeros((n, 48), dtype=torch.uint8, device="cuda")
    tracer.camera_rays_device(rays.data_ptr())
    tracer.trace_rays_device(rays.data_ptr(), n, pkg.RAY_PRIMARY, hits.data_ptr())
    records = [torch.zeros((n, 64), dtype=torch.uint8, device="cuda") for _ in range(2)]
    out_rgb, out_var, out_valid = torch.zeros((n, 3), device="cuda"), torch.zeros((n,), device="cuda"), torch.zeros((n,), dtype=torch.uint8, device="cuda")
    pose = pkg.make_pose(*hs.camera())
    prim = lambda prev, nxt: tracer.temporal_device(t, width, height, pose if prev is not None else None, prev.data_ptr() if prev is not None else None,
                                                    total.data_ptr(), sq.data_ptr(), counts.data_ptr(), hits.data_ptr(), nxt.data_ptr(), out_rgb.data_ptr(),
                                                    d_out_var_ptr=out_var.data_ptr(), d_out_valid_ptr=out_valid.data_ptr())
    prim(None, records[0])
    torch.cuda.synchronize()
    entry["a_temporal_device_no_history"] = median_of(lambda: prim(None, records[1]))
    entry["a_temporal_device"] = median_of(lambda: prim(records[0], records[1]))
    entry["a_share_of_pixels_with_four_taps"] = float((out_valid == 4).float().mean().item())
    src, dst = torch.zeros((107 * n,), dtype=torch.uint8, device="cuda"), torch.zeros((107 * n,), dtype=torch.uint8, device="cuda")
    entry["a_copy_of_107_bytes_a_pixel"] = median_of(lambda: dst.copy_(src))
    entry["a_bytes_moved"] = 213 * n
    print("%dx%d" % (width, height), json.dumps(entry), flush=True)
    tracer.close()
    return entry


for size in args.sizes.split(","):
    w, h = (int(v) for v in size.split("x"))
    result["sizes"][size] = measure(w, h)
if args.bench_roots:
    roots = [os.path.abspath(r) for r in args.bench_roots.split(",")]
    runs = {r: [] for r in roots}
    for _ in range(args.bench_runs):
        for r in roots:   # a fresh process each: the benchmark of that checkout's own library
            p = subprocess.run([sys.executable, os.path.join(r, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline"], cwd=r, capture_output=True,
                               text=True, timeout=300)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')]
            if p.returncode != 0 or not line:
                raise SystemExit("bench.py of %s failed: %s" % (r, p.stderr[-2000:]))
            j = json.loads(line[-1])
            runs[r].append({"value": j["value"], "unit": j.get("unit"), "ms_per_step": j.get("ms_per_step")})
            print("bench", r, runs[r][-1], flush=True)
    result["d_bench_alternating"] = {"parent": runs[roots[0]], "this_tree": runs[roots[1]]}
print(json.dumps(result))
if args.out:
    json.dump(result, open(args.out, "w"), indent=1)
