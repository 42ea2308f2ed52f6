"""Dev helper (GPU box): what lightmap baking costs.  Two meshes -- the HW14-like scene's largest mesh (the knot, full detail) and the HW12-like
scene's floor quad, whose UVs fill the whole map -- at 256 x 256, 1024 x 1024 and 2048 x 2048, warm context, HIP events, median of --repeats
after --warmup calls, one session:
  (a) crt_bake_texels_device (the rasteriser's two launches and the records) beside a device-to-device copy of the bytes it must move: the
      owner plane written and read (8), a record (48) and a ray (24) a texel, 80 a texel: a copy of 40 bytes a texel; and
      crt_bake_dilate_device with two passes (no copy back), halved, beside a copy of the 13 bytes a texel a pass reads and writes
  (b) the whole crt_bake_lightmap (no GI, max_depth 5, dilate 2, no host outputs) beside crt_shoot_rays_device of the same probe rays alone,
      and crt_bake_stats' raster_ms (rasteriser, records, the count's readback, compaction) and shoot_ms
  (c) with --bench-roots PARENT,THIS: `bench.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline` of each root, alternating, --bench-runs
      times (no frame code object changed: the ranges should overlap)
usage: python tools/bake_time.py --out profiles/bake.json [--bench-roots PARENT,.]"""
import argparse, ctypes as C, importlib, json, os, subprocess, sys
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--sizes", default="256,1024,2048")
ap.add_argument("--out", default="")
ap.add_argument("--commit", default="")
ap.add_argument("--bench-roots", default="", help="two checkouts, comma-separated: the parent's and this tree's")
ap.add_argument("--bench-runs", type=int, default=3)
args = ap.parse_args()
sys.path.insert(0, args.root)
import torch
pkg = importlib.import_module("course-assignment-danielhalachev_amd"); sc = pkg.scenes
DEPTH, OFFSET = 5, 1e-3
MESHES = [("hw14_knot", "hw14", 6), ("hw12_floor", "hw12", 0)]


def commit():
    if args.commit:
        return args.commit
    try:
        return subprocess.check_output(["git", "-C", args.root, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        return "unknown"


torch.zeros(1, device="cuda")
stream = torch.cuda.current_stream()


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


def copy_of(n_bytes):
    src, dst = torch.zeros((n_bytes,), dtype=torch.uint8, device="cuda"), torch.zeros((n_bytes,), dtype=torch.uint8, device="cuda")
    return median_of(lambda: dst.copy_(src))


def measure(tracer, mesh, size):
    n = size * size
    entry = {"texels": n}
    bake = pkg.make_bake(mesh=mesh, width=size, height=size, probe_offset=OFFSET)
    texels = torch.zeros((n, 48), dtype=torch.uint8, device="cuda")
    rays = torch.zeros((n, 6), device="cuda")
    work = torch.zeros((pkg.Tracer.bake_work_bytes(size, size),), dtype=torch.uint8, device="cuda")
    call = lambda: tracer.bake_texels_device(bake, texels.data_ptr(), rays.data_ptr(), work.data_ptr())
    call()
    torch.cuda.synchronize()
    entry["a_bake_texels_device"] = median_of(call)
    entry["a_copy_of_40_bytes_a_texel"] = copy_of(40 * n)
    rgb, status = torch.zeros((n, 3), device="cuda"), torch.zeros((n,), dtype=torch.uint8, device="cuda")
    status.copy_(texels[:, 40])   # the records' status word, low byte
    entry["share_covered"] = float((status == 1).float().mean().item())
    two = median_of(lambda: tracer.bake_dilate_device(size, size, 2, rgb.data_ptr(), status.data_ptr(), work.data_ptr()))
    entry["a_one_dilation_pass"] = {k: v / 2 for k, v in two.items()}
    entry["a_copy_of_13_bytes_a_texel"] = copy_of(13 * n)
    # (b) the whole call, and the query of its probe rays alone
    L = pkg.lib()
    o = pkg.make_options(max_depth=DEPTH)
    whole = lambda: tracer._check(L.crt_bake_lightmap(tracer.ctx, C.byref(bake), C.byref(o), None, None, None, None))
    whole()
    entry["b_bake_lightmap"] = median_of(whole)
    st = tracer.bake_stats()
    entry["b_stats_of_the_last_call"] = {"covered": int(st.covered), "dilated": int(st.dilated), "raster_ms": st.raster_ms, "shoot_ms": st.shoot_ms,
                                         "total_ms": st.total_ms}
    covered = (texels[:, 40] == 1)
    probes = rays[covered].contiguous()
    out = torch.zeros((len(probes), 3), device="cuda")
    shoot = lambda: tracer.shoot_rays_device(probes.data_ptr(), len(probes), out.data_ptr(), ray_type=pkg.RAY_REFLECTION, max_depth=DEPTH)
    shoot()
    entry["b_shoot_rays_device_alone"] = median_of(shoot)
    return entry


result = {"max_depth": DEPTH, "probe_offset": OFFSET, "repeats": args.repeats, "warmup": args.warmup, "commit": commit(), "csrc_sha256": pkg.csrc_sha256(),
          "device": torch.cuda.get_device_name(0), "meshes": {}}
for name, scene_name, mesh in MESHES:
    scene = sc.make(scene_name, width=256, height=144)
    if scene_name == "hw14":   # the generator drops this scene's UVs: the knot's are put back
        scene["objects"][mesh] = sc.torus_knot(6, (0.0, -0.05, -4.6), 0.82, 1000, 100, seed=14)
    folder = ""
    if scene.get("textures"):
        import tempfile
        folder = tempfile.mkdtemp()
        sc.write_bitmaps(scene, folder)
    tracer = pkg.Tracer(pkg.Scene(json_text=sc.to_json(scene), folder=folder))
    result["meshes"][name] = {"triangles": int(len(scene["objects"][mesh]["triangles"]))}
    for size in (int(s) for s in args.sizes.split(",")):
        result["meshes"][name][str(size)] = measure(tracer, mesh, size)
        print(name, size, json.dumps(result["meshes"][name][str(size)]), flush=True)
    tracer.close()

if args.bench_roots:
    roots = [os.path.abspath(r) for r in args.bench_roots.split(",")]
    got = {r: [] for r in roots}
    for _ in range(args.bench_runs):
        for r in roots:
            p = subprocess.run([sys.executable, os.path.join(r, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline"], cwd=r,
                               capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit("bench.py of %s failed: %s" % (r, p.stderr[-2000:]))
            j = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')][-1])
            got[r].append({"value": j["value"], "unit": j.get("unit"), "ms_per_step": j.get("ms_per_step")})
            print(r, got[r][-1], flush=True)
    result["c_bench_alternating"] = {"parent": got[roots[0]], "this_tree": got[roots[1]]}
print(json.dumps(result))
if args.out:
    json.dump(result, open(args.out, "w"), indent=1)
