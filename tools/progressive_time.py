"""Dev helper (GPU box): what a progressive sample pass costs beside the one-shot GI frame it adds up to.  HW14, full detail, at 960x540,
max_depth 3, gi_sample_size 2, warm context, HIP events, median of --repeats after --warmup:
  (p) crt_render_progressive, one sample a call, samples --warmup .. --warmup + --repeats - 1 of one continuing frame: events on the
      caller's stream around each call (the call returns when its mean is in the colour buffer, so the events span the sample: the rays
      and keys, the level-synchronous GI query with its host waits, the fold), and crt_get_shoot_stats' kernel_ms of the same calls;
      the device memory a fresh context takes for it (hipMemGetInfo before and after: query scratch, sample arrays and the sum)
  (f) the GI frame of the same camera, options and seed at rays_per_pixel 1, 4 and 16: device time (crt_kernel_times_ms [0]) per frame and
      per sample, crt_stats.queue_bytes and fallback_frames, and the device memory a fresh context takes for it
usage: python tools/progressive_time.py --out profiles/progressive.json
       python tools/progressive_time.py --frame-only --root PARENT_CHECKOUT --out profiles/progressive.json   (the parent's frames, same session:
       written under "frame"; the first command's result is kept)"""
import argparse, importlib, json, os, subprocess, sys
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default="")
ap.add_argument("--frame-only", action="store_true")
ap.add_argument("--commit", default="", help="recorded with the numbers (default: git rev-parse HEAD in --root, if that works)")
args = ap.parse_args()
sys.path.insert(0, args.root)
import torch
pkg = importlib.import_module("course-assignment-danielhalachev_amd"); sc = pkg.scenes
WIDTH, HEIGHT, DEPTH, SAMPLES, SEED = 960, 540, 3, 2, 7
RAYS_PER_PIXEL = (1, 4, 16)


def commit():
    if args.commit:
        return args.commit
    try:
        return subprocess.check_output(["git", "-C", args.root, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        return "unknown"


def free_bytes():
    torch.cuda.synchronize()
    return int(torch.cuda.mem_get_info()[0])


scene = sc.make("hw14", width=WIDTH, height=HEIGHT)
hs = pkg.Scene(json_text=sc.to_json(scene))
torch.zeros(1, device="cuda")
head = {"scene": "hw14 full detail %dx%d" % (hs.width, hs.height), "max_depth": DEPTH, "gi_sample_size": SAMPLES, "gi_seed": SEED,
        "repeats": args.repeats, "warmup": args.warmup, "commit": commit(), "csrc_sha256": pkg.csrc_sha256(), "device": torch.cuda.get_device_name(0)}


def frames():
    """the one-shot frames: a fresh context for each rays_per_pixel, so that queue_bytes and the memory are that frame's"""
    out = {}
    for rpp in RAYS_PER_PIXEL:
        options = pkg.make_options(DEPTH, use_gi=True, gi_sample_size=SAMPLES, rays_per_pixel=rpp, gi_seed=SEED)
        before = free_bytes()
        tracer = pkg.Tracer(hs)
        created = free_bytes()
        entry = {"rays_per_pixel": rpp}
        try:
            for _ in range(args.warmup + args.repeats):
                tracer.render(options=options)
            times = [t[0] for t in tracer.kernel_times_ms()[-args.repeats:]]
            st = tracer.stats()
            entry.update(frame_ms=float(np.median(times)), frame_ms_min=float(min(times)), ms_per_sample=float(np.median(times)) / rpp,
                         queue_bytes=int(st.queue_bytes), fallback_frames=int(st.fallback_frames), queue_regrows=int(st.queue_regrows),
                         device_bytes_for_the_frames=created - free_bytes(), device_bytes_of_the_context=before - created)
        except pkg.CrtError as e:   # a frame that does not fit is the finding
            entry["error"] = str(e)
        out[str(rpp)] = entry
        print("frame", entry, flush=True)
        tracer.close()
    return out


def progressive():
    options = pkg.make_options(DEPTH, use_gi=True, gi_sample_size=SAMPLES, rays_per_pixel=1, gi_seed=SEED)
    tracer = pkg.Tracer(hs)
    created = free_bytes()
    L, stream = pkg.lib(), torch.cuda.current_stream()
    ms, kernel_ms, generations = [], [], []
    total = args.warmup + args.repeats
    mean = np.zeros((hs.height, hs.width, 3), dtype=np.float32)
    for s in range(total):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        tracer._check(L.crt_render_progressive(tracer.ctx, options, s, 1, mean.ctypes.data if s + 1 == total else None))   # (the last call copies the mean out)
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
        kernel_ms.append(float(tracer.shoot_stats().kernel_ms))
        generations.append(tracer.query_scratch_generation())
    st = tracer.shoot_stats()
    entry = {"ms_per_sample": float(np.median(ms[args.warmup:])), "ms_per_sample_min": float(min(ms[args.warmup:])),
             "ms_first_sample": float(ms[0]), "query_kernel_ms_per_sample": float(np.median(kernel_ms[args.warmup:])),
             "samples": tracer.progressive_samples(), "levels": int(st.levels), "level_rays_last_sample": [int(x) for x in st.level_rays[:st.levels]],
             "scratch_generation_after_sample_1": generations[1], "scratch_generation_after_last_sample": generations[-1],
             "device_bytes_scratch_samples_and_sum": created - free_bytes(), "sum_bytes": hs.width * hs.height * 12,
             "queue_bytes": int(tracer.stats().queue_bytes)}
    # the frame so far is the one-shot frame with as many rays per pixel, bit for bit
    one_shot = pkg.Tracer(hs)
    frame = one_shot.render(options=pkg.make_options(DEPTH, use_gi=True, gi_sample_size=SAMPLES, rays_per_pixel=total, gi_seed=SEED))
    entry["equals_the_one_shot_frame_of_%d_rays_per_pixel_bit_for_bit" % total] = bool(np.array_equal(mean.view(np.uint32), frame.view(np.uint32)))
    entry["one_shot_fallback_frames"] = int(one_shot.stats().fallback_frames)
    one_shot.close()
    print("progressive", entry, flush=True)
    tracer.close()
    return entry


result = {}
if args.out and os.path.exists(args.out):
    result = json.load(open(args.out))
if args.frame_only:
    result["frame"] = dict(head, frames=frames())
else:
    result = dict(head, progressive=progressive(), frames_of_this_tree=frames(), **({"frame": result["frame"]} if "frame" in result else {}))
print(json.dumps(result))
if args.out:
    json.dump(result, open(args.out, "w"), indent=1)
