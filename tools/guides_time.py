"""Times the chain guides on one GPU: HW14, full detail, at 960x540 and 1920x1080, HIP events, median of 20 calls
after 5 warm-up calls, everything in one session.
  * crt_guide_rays_device at 0, 1 and 8 bounces for the camera's rays, against crt_trace_rays_device of the same rays -- this tree's and,
    with --parent-root, the parent checkout's (a child process of this tool with --trace-only);
  * guide_step alone: the library has no entry that launches it without a trace, so it is the difference "0 bounces - this tree's trace" --
    one guide_step launch over all n rays and the one query_reset launch ahead of the call --, against a device-to-device copy of the bytes
    the kernel moves at level 0 (it reads a 24-byte ray and a 48-byte record and writes a 48-byte record, a status byte and a 24-byte ray: a
    copy of 72 n bytes reads and writes as much);
  * crt_render_denoised on a 2-sample adaptive frame, depth 3, without and with 4-bounce chain guides: the call with kept guides, and the
    frame's first call, which traces them (wall time: the call waits for its result);
  * with --parent-root: bench.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline of the parent and of this tree, alternating, three times.
usage: python tools/guides_time.py [--out profiles/guides.json] [--parent-root DIR] [--sizes 960x540,1920x1080]"""
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, CALLS = 5, 20


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def median_ms(torch, call):
    for _ in range(WARM):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return round(statistics.median(times), 4)


def wall_ms(call, calls=CALLS, warm=WARM):
    for _ in range(warm):
        call()
    times = []
    for _ in range(calls):
        t = time.perf_counter()
        call()
        times.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(times), 4)


def measure(root, width, height, trace_only):
    import torch
    sys.path.insert(0, root)
    pkg = importlib.import_module("course-assignment-danielhalachev_amd")
    scene = pkg.scenes.make("hw14", width=width, height=height)
    tracer = pkg.Tracer(pkg.Scene(json_text=pkg.scenes.to_json(scene)))
    n = width * height
    rays = torch.zeros((n, 6), dtype=torch.float32, device="cuda")
    hits = torch.zeros((n, 48), dtype=torch.uint8, device="cuda")
    tracer.camera_rays_device(rays.data_ptr())
    torch.cuda.synchronize()
    out = {"rays": n, "trace_rays_device_ms": median_ms(torch, lambda: tracer.trace_rays_device(rays.data_ptr(), n, pkg.RAY_PRIMARY, hits.data_ptr()))}
    if trace_only:
        return out
    status = torch.zeros((n,), dtype=torch.uint8, device="cuda")
    last = torch.zeros((n, 6), dtype=torch.float32, device="cuda")
    work = torch.zeros((tracer.guide_work_bytes(n),), dtype=torch.uint8, device="cuda")
    for bounces in (0, 1, 8):
        out["guide_rays_device_%d_ms" % bounces] = median_ms(torch, lambda: tracer.guide_rays_device(
            rays.data_ptr(), n, pkg.RAY_PRIMARY, bounces, hits.data_ptr(), work.data_ptr(), d_status_ptr=status.data_ptr(), d_last_rays_ptr=last.data_ptr()))
        torch.cuda.synchronize()
        s = status.cpu().numpy()
        out["bounces_histogram_%d" % bounces] = [int(c) for c in __import__("numpy").bincount(s & 63)]
    out["trace_rays_device_again_ms"] = median_ms(torch, lambda: tracer.trace_rays_device(rays.data_ptr(), n, pkg.RAY_PRIMARY, hits.data_ptr()))
    out["guide_step_level0_and_reset_ms"] = round(out["guide_rays_device_0_ms"] - min(out["trace_rays_device_ms"], out["trace_rays_device_again_ms"]), 4)
    a, b = torch.zeros((72 * n,), dtype=torch.uint8, device="cuda"), torch.zeros((72 * n,), dtype=torch.uint8, device="cuda")
    out["copy_72n_bytes_ms"] = median_ms(torch, lambda: b.copy_(a))
    # the frame call: a finished 2-sample adaptive frame, denoised again and again (the frame is left as it was)
    options = pkg.make_options(3, use_gi=True, gi_sample_size=2, rays_per_pixel=1, gi_seed=9)
    adaptive, denoise = pkg.make_adaptive(min_samples=2, max_samples=2, threshold=0.05, floor=1e-4), pkg.make_denoise()
    for tag, bounces in (("first_hit", 0), ("chain_4", 4)):
        tracer.set_guide_bounces(bounces)
        firsts = []
        for _ in range(3):
            tracer.render_adaptive(options, adaptive)
            t = time.perf_counter()
            tracer.render_denoised(denoise)
            firsts.append((time.perf_counter() - t) * 1e3)
        out["render_denoised_%s_first_call_ms" % tag] = round(statistics.median(firsts), 4)
        out["render_denoised_%s_ms" % tag] = wall_ms(lambda: tracer.render_denoised(denoise))
    tracer.set_guide_bounces(0)
    return out


def bench(root):
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline"], cwd=root,
                       capture_output=True, text=True, timeout=280)
    for line in r.stdout.splitlines():
        if line.startswith('{"metric"'):
            return json.loads(line)["value"]
    raise RuntimeError("bench.py in %s: %s" % (root, r.stderr[-400:]))


def main():
    sizes = [tuple(int(v) for v in s.split("x")) for s in arg("--sizes", "960x540,1920x1080").split(",")]
    if "--trace-only" in sys.argv:
        print(json.dumps({"%dx%d" % s: measure(arg("--root"), s[0], s[1], True) for s in sizes}))
        return
    parent = os.path.abspath(arg("--parent-root")) if arg("--parent-root") else None
    result = {"how": "tools/guides_time.py: HW14 full detail, HIP events, median of %d after %d warm-up calls, one session" % (CALLS, WARM), "sizes": {}}
    for s in sizes:
        result["sizes"]["%dx%d" % s] = measure(ROOT, s[0], s[1], False)
        print("%dx%d" % s, json.dumps(result["sizes"]["%dx%d" % s]), flush=True)
    if parent:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--trace-only", "--root",
                            parent, "--sizes", arg("--sizes", "960x540,1920x1080")], capture_output=True, text=True, timeout=280, cwd=parent)
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-600:])
        result["parent_trace_rays_device"] = json.loads(r.stdout.strip().splitlines()[-1])
        print("parent", json.dumps(result["parent_trace_rays_device"]), flush=True)
        result["bench_mpixels_per_s"] = {"parent": [], "this_tree": []}
        for _ in range(3):
            result["bench_mpixels_per_s"]["parent"].append(bench(parent))
            result["bench_mpixels_per_s"]["this_tree"].append(bench(ROOT))
            print("bench", json.dumps(result["bench_mpixels_per_s"]), flush=True)
    out = arg("--out")
    if out:
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
