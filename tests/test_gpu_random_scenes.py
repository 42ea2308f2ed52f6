"""The seeded random scenes of tests/random_scene_sets.py on the GPU: frames on every kernel path, the counting build's counters,
further cameras, the ray, lighting and radiance queries, the GI mode (frames, radiance queries, two adaptive passes) and the chain guides
against the CPU oracle bit for bit (NaN equals NaN), and the eight fixture seeds against the real reference's recorded floats
(tests/golden/random_scenes.npz).  Occlusion is compared under the default rule only: the library has no occlusion query under the GI
rule (no mesh skipped); that rule is held to the live reference on the CPU (tests/test_random_scenes_host.py) and runs inside the GI
frames here.  A failure names its seed; narrow it
by hand with random_scene_sets.make(seed, w, h, keep_meshes=[...], keep_lights=[...])."""
import numpy as np
import pytest

import query_sets as qs
import random_scene_sets as rss
import shade_sets as ss
from helpers import assert_same_hits, assert_shaded

pytestmark = pytest.mark.gpu

TUNINGS = [None,                                                                  # the defaults: the candidate-filter kernels where the scene has a filter
           dict(bvh=0),                                                           # the reference-order kernels: plan kernels + wave-per-ray kernels
           dict(bvh=0, step_budget=8, shadow_budget=8, level0_budget=8),         # nearly every walk through the wave-per-ray kernels
           dict(mode=1),                                                          # the recursive one-ray-per-lane kernel
           dict(bvh=2),                                                           # the filter kernels' bounds-checked build
           dict(bvh=1, level_queue=258),                                          # every child ray through the level queue
           dict(bvh=1, level_queue=0, side_blocks=0)]                             # one launch per level, no side stream
N_RAYS = 512
_CASES = {}


def tuning_id(t):
    return "defaults" if t is None else ",".join("%s=%s" % kv for kv in t.items())


def case(pkg, scenes, oracle, seed, tmp_path_factory):
    """A seed's scene, its oracle, the oracle's frame and counters, and a tracer with the default tuning: made once."""
    if seed not in _CASES:
        scene = rss.seed_scene(seed)
        folder = str(tmp_path_factory.mktemp("seed%d" % seed))
        scenes.write_bitmaps(scene, folder)
        o = oracle.OracleScene(scenes.to_blob(scene))
        want, counters = o.render(rss.depth_of(scene))
        want.setflags(write=False)
        _CASES[seed] = dict(scene=scene, folder=folder, depth=rss.depth_of(scene), oracle=o, want=want, counters=counters,
                            host=pkg.Scene(json_text=scenes.to_json(scene), folder=folder))
        _CASES[seed]["tracer"] = pkg.Tracer(_CASES[seed]["host"])
    return _CASES[seed]


def query_case(pkg, scenes, oracle, seed, tmp_path_factory):
    c = case(pkg, scenes, oracle, seed, tmp_path_factory)
    if "rays" not in c:
        c["rays"] = rss.rays(c["scene"], seed, N_RAYS, c["oracle"])
        c["rays"].setflags(write=False)
        c["dist"] = rss.distances(seed, N_RAYS)
    return c


# ---- 1. frames, on every kernel path
@pytest.mark.parametrize("tuning", TUNINGS, ids=tuning_id)
@pytest.mark.parametrize("seed", rss.SEEDS)
def test_frame_equals_the_oracle_on_every_kernel_path(pkg, scenes, oracle, seed, tuning, tmp_path_factory):
    c = case(pkg, scenes, oracle, seed, tmp_path_factory)
    tracer = pkg.Tracer(c["host"], tuning=pkg.make_tuning(**tuning)) if tuning else c["tracer"]
    for frame in ("first", "second"):       # the second frame of a context sizes (or leaves out) launches by the first frame's counters
        rss.assert_same_frame(tracer.render(max_depth=c["depth"]), c["want"], "seed %d, tuning %s, %s frame" % (seed, tuning_id(tuning), frame))
        assert tracer.stats().fallback_frames == 0, "seed %d, tuning %s, %s frame" % (seed, tuning_id(tuning), frame)


def test_the_filter_keeps_three_quarters_of_the_scenes(pkg, scenes, oracle, tmp_path_factory):
    kept = []
    for seed in rss.SEEDS:
        c = case(pkg, scenes, oracle, seed, tmp_path_factory)
        k = c["tracer"].kernels()
        filtered = not k["filter"].startswith("none")
        assert filtered == rss.filter_accepts(pkg, scenes, c["scene"], c["folder"]), "seed %d: %r" % (seed, k)   # the device's filter is the host build's
        assert k["level0"].startswith("bvh_trace_") == filtered, "seed %d: %r" % (seed, k)
        kept += [seed] if filtered else []
    assert 4 * len(kept) >= 3 * len(rss.SEEDS), kept


@pytest.mark.parametrize("seed", rss.SEEDS)
def test_counting_build_equals_the_oracle_s_counters(pkg, scenes, oracle, seed, tmp_path_factory):
    c = case(pkg, scenes, oracle, seed, tmp_path_factory)
    got = c["tracer"].render(max_depth=c["depth"], counters=True)
    st = c["tracer"].stats()
    rss.assert_same_frame(got, c["want"], "seed %d, counting build" % seed)
    assert st.counters_valid == 1 and st.counters() == c["counters"], "seed %d: %r, expected %r" % (seed, st.counters(), c["counters"])


# ---- 2. the real reference's floats
@pytest.mark.parametrize("seed", rss.FIXTURE_SEEDS)
def test_fixture_seeds_equal_the_reference(pkg, scenes, seed, tmp_path):
    fx = rss.load_fixture()[seed]
    scene = rss.make(seed, *rss.FIXTURE_SIZE)
    scenes.write_bitmaps(scene, str(tmp_path))
    tracer = pkg.Tracer(pkg.Scene(json_text=scenes.to_json(scene), folder=str(tmp_path)))
    depth, rays = int(np.ravel(fx["depth"])[0]), np.ascontiguousarray(fx["rays"])
    rss.assert_same_frame(tracer.render(max_depth=depth), fx["frame"], "seed %d: the reference's frame" % seed)
    for t in rss.HIT_TYPES:
        assert_same_hits(tracer.trace_rays(rays, t), fx["hits_%d" % t].astype(pkg.HIT_DTYPE), "seed %d: the reference's hits of type %d" % (seed, t))
    bad = np.flatnonzero(tracer.occluded_rays(rays, fx["dist"]) != fx["occ"])
    assert bad.size == 0, "seed %d: occlusion differs from the reference's for %d rays, first %d" % (seed, bad.size, bad[0])
    for k, t in enumerate(rss.RAY_TYPES):
        rss.assert_same_frame(tracer.shoot_rays(rays, t, max_depth=depth), fx["shoot"][k], "seed %d: the reference's shootRay, type %d" % (seed, t))


# ---- 3. further cameras, the scene resident
@pytest.mark.parametrize("seed", rss.SEEDS)
def test_three_more_cameras(pkg, scenes, oracle, seed, tmp_path_factory):
    c = case(pkg, scenes, oracle, seed, tmp_path_factory)
    tracer, o = c["tracer"], c["oracle"]
    rng = np.random.default_rng([seed, 0xCA])
    try:
        for k in range(3):
            pos, mat = rss.random_camera(rng, c["scene"])
            tracer.set_camera(pos, mat)
            o.set_camera(pos, mat)
            rss.assert_same_frame(tracer.render(max_depth=c["depth"]), o.render(c["depth"])[0], "seed %d, camera %d (%r, %r)" % (seed, k, pos.tolist(), mat.tolist()))
            assert tracer.stats().fallback_frames == 0
    finally:
        for x in (tracer, o):
            x.set_camera(c["scene"]["camera"]["position"], c["scene"]["camera"]["matrix"])


# ---- 4. queries
def device_hits(pkg, tracer, rays, ray_type):
    import torch
    d_rays = torch.from_numpy(np.array(rays)).cuda()
    d_hits = torch.full((len(rays) + 1, 48), 0xA5, dtype=torch.uint8, device="cuda")      # (one record more: must stay untouched)
    torch.cuda.synchronize()
    tracer.trace_rays_device(d_rays.data_ptr(), len(rays), ray_type, d_hits.data_ptr())
    torch.cuda.synchronize()
    hits = d_hits.cpu().numpy()
    assert np.all(hits[len(rays):] == 0xA5), "written past the end"
    return hits[:len(rays)].view(pkg.HIT_DTYPE).reshape(-1)


@pytest.mark.parametrize("seed", rss.SEEDS)
def test_closest_hits_and_occlusion(pkg, scenes, oracle, seed, tmp_path_factory):
    import torch
    c = query_case(pkg, scenes, oracle, seed, tmp_path_factory)
    tracer, o, rays, dist = c["tracer"], c["oracle"], c["rays"], c["dist"]
    for t in rss.RAY_TYPES:
        want = qs.oracle_hits(o, c["scene"], rays, t, pkg.HIT_DTYPE)
        assert_same_hits(tracer.trace_rays(rays, t), want, "seed %d: trace_rays type %d" % (seed, t))
        assert_same_hits(device_hits(pkg, tracer, rays, t), want, "seed %d: trace_rays_device type %d" % (seed, t))
        if t == qs.RAY_REFLECTION:
            assert int(want["hit"].sum()) >= 40, "seed %d: the rays must meet the scene" % seed
            c["hits"] = want
    for what, limit in (("per-ray limits", dist), ("no limit", np.full(len(rays), np.inf, dtype=np.float32))):
        want = qs.oracle_occluded(o, rays, limit)
        bad = np.flatnonzero(tracer.occluded_rays(rays, limit) != want)
        assert bad.size == 0, "seed %d: occluded_rays, %s: %d rays differ, first %d" % (seed, what, bad.size, bad[0])
        d_rays, d_dist = torch.from_numpy(np.array(rays)).cuda(), torch.from_numpy(np.array(limit)).cuda()
        d_occ = torch.full((len(rays) + 1,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        tracer.occluded_rays_device(d_rays.data_ptr(), d_dist.data_ptr(), len(rays), d_occ.data_ptr())
        torch.cuda.synchronize()
        occ = d_occ.cpu().numpy()
        assert occ[-1] == 0xA5 and np.array_equal(occ[:-1].astype(bool), want), "seed %d: occluded_rays_device, %s" % (seed, what)


@pytest.mark.parametrize("seed", rss.SEEDS)
def test_radiance_queries(pkg, scenes, oracle, seed, tmp_path_factory):
    import torch
    c = query_case(pkg, scenes, oracle, seed, tmp_path_factory)
    tracer, o, rays = c["tracer"], c["oracle"], c["rays"]
    d_rays = torch.from_numpy(np.array(rays)).cuda()
    for depth in sorted({1, c["depth"]}):
        for t in rss.RAY_TYPES:
            want = np.array([o.shoot(r[:3], r[3:], t, 0, depth) for r in rays], dtype=np.float32)
            what = "seed %d: shoot_rays type %d depth %d" % (seed, t, depth)
            rss.assert_same_frame(tracer.shoot_rays(rays, t, max_depth=depth), want, what)
            d_rgb = torch.full((len(rays) + 1, 3), float("nan"), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            tracer.shoot_rays_device(d_rays.data_ptr(), len(rays), d_rgb.data_ptr(), t, max_depth=depth)
            torch.cuda.synchronize()
            rgb = d_rgb.cpu().numpy()
            assert np.all(np.isnan(rgb[len(rays):])), what + ": written past the end"
            rss.assert_same_frame(rgb[:len(rays)], want, what + ", device variant")


@pytest.mark.parametrize("seed", rss.SEEDS)
def test_direct_lighting_of_the_oracle_s_records(pkg, scenes, oracle, seed, tmp_path_factory):
    """shade_hits on the oracle's hit records and light_points on their points and normals.  The expected colour of a record is shootRay
    at max_depth 0 of its ray, so only rays whose direction is a fixed point of shootRay's normalisation are used (tests/shade_sets.py);
    light_points is one channel of the same scene with every diffuse albedo white."""
    c = query_case(pkg, scenes, oracle, seed, tmp_path_factory)
    tracer, o, scene = c["tracer"], c["oracle"], c["scene"]
    rays = ss.fixed_point_rays(c["rays"])
    assert len(rays) >= N_RAYS // 2
    hits = qs.oracle_hits(o, scene, rays, qs.RAY_REFLECTION, pkg.HIT_DTYPE)
    status = ss.expected_status(pkg, scene, hits)
    rgb, got_status = tracer.shade_hits(hits)
    assert_shaded(pkg, rgb, got_status, status, ss.oracle_colours(o, rays), "seed %d: shade_hits" % seed)
    finite = np.isfinite(hits["point"]).all(axis=1) & np.isfinite(hits["normal"]).all(axis=1)
    diffuse = (status == pkg.SHADE_DIFFUSE) & finite
    if diffuse.any():
        white = oracle.OracleScene(scenes.to_blob(ss.white_scene(scene)))
        want = ss.oracle_colours(white, rays[diffuse])
        got = tracer.light_points(hits["point"][diffuse].copy(), hits["normal"][diffuse].copy())
        rss.assert_same_frame(got[:, None], want[:, :1], "seed %d: light_points" % seed)


# ---- 5. the GI mode
@pytest.mark.parametrize("samples", [1, 2])
@pytest.mark.parametrize("seed", rss.GI_SEEDS)
def test_gi_frame_and_gi_radiance_queries(pkg, scenes, oracle, seed, samples, tmp_path_factory):
    """the GI frame (two rays per pixel) and shoot_rays_gi for all the seed's rays under random keys, every ray type, at the seed's depth"""
    import torch
    c = query_case(pkg, scenes, oracle, seed, tmp_path_factory)
    tracer, o, depth, rays = c["tracer"], c["oracle"], c["depth"], c["rays"]
    fields = dict(use_gi=1, gi_sample_size=samples, rays_per_pixel=2, gi_seed=1000 + seed)
    options = pkg.make_options(depth, **dict(fields, use_gi=True))
    want, _ = o.render(options=oracle.make_options(depth, **fields))
    rss.assert_same_frame(tracer.render(options=options), want, "seed %d: GI frame, %d samples, depth %d" % (seed, samples, depth))
    keys = np.random.default_rng([seed, samples]).integers(0, 1 << 32, len(rays), dtype=np.uint64).astype(np.uint32)
    d_rays, d_keys = torch.from_numpy(np.array(rays)).cuda(), torch.from_numpy(keys.view(np.int32).copy()).cuda()
    for t in rss.RAY_TYPES:
        what = "seed %d: shoot_rays_gi type %d, %d samples, depth %d" % (seed, t, samples, depth)
        want = o.shoot_gi(rays, keys, t, oracle.make_options(depth, **fields))
        rss.assert_same_frame(tracer.shoot_rays_gi(rays, keys, t, options), want, what)
        d_rgb = torch.full((len(rays) + 1, 3), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        tracer.shoot_rays_gi_device(d_rays.data_ptr(), len(rays), d_rgb.data_ptr(), d_keys.data_ptr(), t, options)
        torch.cuda.synchronize()
        rgb = d_rgb.cpu().numpy()
        assert np.all(np.isnan(rgb[len(rays):])), what + ": written past the end"
        rss.assert_same_frame(rgb[:len(rays)], want, what + ", device variant")


@pytest.mark.parametrize("samples", [1, 2])
@pytest.mark.parametrize("seed", rss.GI_SEEDS)
def test_two_adaptive_passes_equal_the_oracle_s_fold(pkg, scenes, oracle, seed, samples, tmp_path_factory):
    """render_adaptive with min_samples 1 and max_samples 2: two passes.  The oracle shoots sample 0 and sample 1 of every pixel
    (guide_sets.oracle_sample_colours: key mix(mix(seed, p), s), sample 0 through the centre, sample 1 jittered); the stopping rule restated
    in numpy (adaptive_sets.run) says which pixels take the second sample, and a pixel with k samples holds the fold of its first k
    colours (progressive_sets.fold).  Compared as float values: the fold's `0 + colour` turns a -0 into +0 and changes nothing else."""
    import adaptive_sets as ads
    import guide_sets as g
    import progressive_sets as ps
    from shoot_gi_sets import assert_same_values
    c = case(pkg, scenes, oracle, seed, tmp_path_factory)
    tracer, o, depth, gi_seed = c["tracer"], c["oracle"], c["depth"], 2000 + seed
    a = pkg.make_adaptive(min_samples=1, max_samples=2, threshold=0.1, floor=1e-4)
    rgb, counts = tracer.render_adaptive(ps.frame_options(pkg, depth, samples, 1, seed=gi_seed), a)
    assert tracer.progressive_active() == 0
    colours = g.oracle_sample_colours(o, oracle, 2, depth=depth, gi_samples=samples, seed=gi_seed)
    want = ads.run(colours, a)
    pixels = o.width * o.height
    bad = np.flatnonzero(counts.reshape(pixels) != want["counts"])
    assert bad.size == 0, "seed %d, %d samples: the sample counts of %d pixels differ, first: row %d col %d got %d want %d" % (
        seed, samples, bad.size, bad[0] // o.width, bad[0] % o.width, counts.reshape(pixels)[bad[0]], want["counts"][bad[0]])
    for k in (1, 2):
        at = want["counts"] == k
        assert_same_values(rgb.reshape(pixels, 3)[at], ps.fold(colours[:k])[1][at], "seed %d, %d samples: the %d pixels with %d samples" % (seed, samples, int(at.sum()), k))


# ---- 6. chain guides
@pytest.mark.parametrize("seed", rss.GUIDE_SEEDS)
def test_chain_guides_equal_the_host_walk(pkg, scenes, oracle, seed, tmp_path_factory):
    """crt_guide_rays_device with 3 bounces for the camera's rays and the seed's query rays against the host walk over OracleScene.trace
    (tests/guide_sets.py), on the seeds whose primary rays meet a mirror or glass."""
    import torch
    import guide_sets as g
    import shoot_gi_sets as gs
    c = query_case(pkg, scenes, oracle, seed, tmp_path_factory)
    tracer, o, scene = c["tracer"], c["oracle"], c["scene"]
    rays = np.ascontiguousarray(np.concatenate([gs.camera_rays(o), c["rays"]]))
    n, pixels = len(rays), o.width * o.height
    want = g.walk_all(o, scene, rays, qs.RAY_PRIMARY, 3)
    assert int(((want["status"][:pixels] & 63) > 0).sum()) > 0, "seed %d: no mirror or glass in view" % seed
    d_rays = torch.from_numpy(rays).cuda()
    d_hits = torch.full((n + 1, 48), 0xA5, dtype=torch.uint8, device="cuda")
    d_status = torch.full((n + 1,), 0xA5, dtype=torch.uint8, device="cuda")
    d_last = torch.full((n + 1, 6), float("nan"), dtype=torch.float32, device="cuda")
    d_work = torch.zeros(tracer.guide_work_bytes(n) + 16, dtype=torch.uint8, device="cuda")
    work = (d_work.data_ptr() + 15) // 16 * 16
    torch.cuda.synchronize()
    tracer.guide_rays_device(d_rays.data_ptr(), n, qs.RAY_PRIMARY, 3, d_hits.data_ptr(), work, d_status.data_ptr(), d_last.data_ptr())
    torch.cuda.synchronize()
    hits, status, last = d_hits.cpu().numpy(), d_status.cpu().numpy(), d_last.cpu().numpy()
    assert np.all(hits[n:] == 0xA5) and status[n] == 0xA5 and np.all(np.isnan(last[n:])), "seed %d: written past the end" % seed
    bad = np.flatnonzero(status[:n] != want["status"])
    assert bad.size == 0, "seed %d: the status of %d rays differs, first %d: got %d want %d" % (seed, bad.size, bad[0], status[bad[0]], want["status"][bad[0]])
    rss.assert_same_frame(last[:n], want["last_rays"], "seed %d: the terminal segments' rays" % seed)
    assert_same_hits(hits[:n].view(pkg.HIT_DTYPE).reshape(-1), want["records"].astype(pkg.HIT_DTYPE), "seed %d: guide records" % seed)
