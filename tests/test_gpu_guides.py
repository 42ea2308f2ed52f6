"""The chain guides on the GPU (include/crt_hip.h, "Chain guides": crt_guide_rays*, crt_set_guide_bounces).  tests/guide_sets.py restates
the rule and tests/test_guides_host.py holds that to the oracle; here the library gives the restatement's records, is pinned to
crt_shoot_rays (itself held to the real reference) with no restatement in between, and the frame calls filter under its guides."""
import ctypes as C

import numpy as np
import pytest

import adaptive_sets as ads
import denoise_sets as dns
import guide_sets as g
import progressive_sets as ps
import shoot_gi_sets as gs
from shoot_gi_sets import W, H, case
from test_gpu_adaptive import sample_colours, settings as adaptive_settings
from test_guides_host import pinned_rays, restated_measure, walks

pytestmark = pytest.mark.gpu
PIXELS = W * H
PRIMARY = 0

_tracers = {}


def tracer_of(pkg, scenes, which):
    """a tracer of one of guide_sets' scenes, made once"""
    if which not in _tracers:
        scene = {"white": g.white_mirror_scene, "wall": g.mirror_wall_scene, "facing": g.facing_mirrors_scene}[which](scenes)
        _tracers[which] = pkg.Tracer(pkg.Scene(json_text=scenes.to_json(scene)))
    return _tracers[which]


@pytest.fixture
def hw11(pkg, scenes, oracle, tmp_path_factory):
    c = case(pkg, scenes, oracle, "hw11", tmp_path_factory)
    c["tracer"].set_camera(*c["tracer"].scene.camera())
    return c


def same_records(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    for field in want.dtype.names:
        a, b = got[field], want[field]
        if a.dtype.kind == "f":
            a, b = a.view(np.uint32), b.view(np.uint32)
        bad = np.flatnonzero((a != b).reshape(len(want), -1).any(axis=1))
        assert bad.size == 0, "%s: %s differs in %d records, first %d: got %r want %r" % (what, field, bad.size, bad[0], got[bad[0]], want[bad[0]])


# ---- 1. max_bounces = 0 is crt_trace_rays
@pytest.mark.parametrize("n", [1, 63, 64, 65, PIXELS])
def test_zero_bounces_is_trace_rays(pkg, hw11, n):
    tracer, rays = hw11["tracer"], hw11["rays"][:n]
    want = tracer.trace_rays(rays, pkg.RAY_PRIMARY)
    got, status, last = tracer.guide_rays(rays, pkg.RAY_PRIMARY, 0)
    assert got.tobytes() == want.tobytes()
    assert np.all((status & 63) == 0) and np.array_equal(last, rays)
    specular = np.array([g.material_of(hw11["scene"], int(m))["type"] in ("reflective", "refractive") for m in want["mesh"]]) & (want["hit"] != 0)
    assert np.array_equal(status, np.where(specular, g.CUT, 0).astype(np.uint8))


def test_no_rays_touch_nothing(pkg, hw11):
    tracer = hw11["tracer"]
    hits = np.full(4, 0xEE, dtype=np.uint8)
    o = pkg.make_options(0)
    assert pkg.lib().crt_guide_rays(tracer.ctx, None, 0, 0, C.byref(o), 4, hits.ctypes.data_as(C.c_void_p), None, None) == 0
    assert pkg.lib().crt_guide_rays_device(tracer.ctx, None, 0, 0, None, 99, None, None, None, None, None) == 0
    assert np.all(hits == 0xEE)


# ---- 2. pinned to the reference with no restatement
def test_the_terminal_hit_shades_to_shoot_rays(pkg, scenes, oracle):
    """white mirrors: shootRay of a ray whose chain is all reflective and ends on a diffuse mesh is the direct light of the terminal hit.
    The rays are the camera's in the form shootRay holds them (guide_sets.fixed_point): the guide call walks a ray as given."""
    tracer = tracer_of(pkg, scenes, "white")
    tracer.set_camera(g.MIRROR_CAMERA[0], gs.look_at(*g.MIRROR_CAMERA))
    w = walks(scenes, oracle, "white", 8, g.MIRROR_CAMERA)
    rays = w["rays"]
    records, status, _ = tracer.guide_rays(rays, pkg.RAY_PRIMARY, 8)
    assert np.array_equal(status, w["walk"]["status"])
    sel = w["fixed"] & (status >= 1) & (status < g.CUT) & w["walk"]["all_reflective"] & (w["walk"]["kinds"] == g.DIFFUSE)
    assert np.array_equal(sel, pinned_rays(w)) and sel.sum() >= 30, sel.sum()
    want = tracer.shoot_rays(rays[sel], pkg.RAY_PRIMARY, max_depth=8)
    got, shade_status = tracer.shade_hits(g.untagged(records[sel], len(w["scene"]["objects"])))
    assert np.all(shade_status == pkg.SHADE_DIFFUSE)
    assert got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), int((got.view(np.uint32) != want.view(np.uint32)).any(axis=1).sum())


# ---- 3. the terminal segment, the bounce count, the tag and the path length
def test_the_chain_is_the_host_walk(pkg, scenes, oracle, hw11):
    import query_sets as qs
    tracer, o, scene, rays = hw11["tracer"], hw11["oracle"], hw11["scene"], hw11["rays"]
    want = g.walk_all(o, scene, rays, PRIMARY, 8)
    records, status, last = tracer.guide_rays(rays, pkg.RAY_PRIMARY, 8)
    assert np.array_equal(status, want["status"])
    assert (status & 63).max() >= 2 and np.any(~want["all_reflective"])   # (through the glass sphere; a miss: the facing mirrors' test)
    assert last.view(np.uint32).tobytes() == want["last_rays"].view(np.uint32).tobytes()
    n_meshes = len(scene["objects"])
    for kind in np.unique(want["last_types"]):   # the oracle's trace of the terminal segment, with its segment's ray type
        at = np.flatnonzero(want["last_types"] == kind)
        traced = qs.oracle_hits(o, scene, last[at], int(kind), g.HIT_DTYPE)
        for field in ("point", "normal", "u", "v", "triangle", "hit"):
            assert records[field][at].tobytes() == traced[field].tobytes(), (int(kind), field)
        assert np.array_equal(g.untagged(records[at], n_meshes)["mesh"], traced["mesh"])
    same_records(records, want["records"], "hw11, 8 bounces")


# ---- 4. cut chains
@pytest.mark.parametrize("bounces", [1, 3, 63])
def test_a_chain_between_two_mirrors_is_cut(pkg, scenes, oracle, bounces):
    tracer, scene, o = tracer_of(pkg, scenes, "facing"), g.facing_mirrors_scene(scenes), g.oracle_scene(scenes, oracle, "facing")
    rays, _ = g.fixed_point(np.array([[0.0, 0.1, 0.0, 1.0, 0.002, 0.001], [0.0, 0.0, 0.0, 0.0, 0.3, -1.0]], dtype=np.float32))
    want = g.walk_all(o, scene, rays, PRIMARY, bounces)
    records, status, last = tracer.guide_rays(rays, pkg.RAY_PRIMARY, bounces)
    assert status[0] == (g.CUT | bounces) and records["hit"][0] == 1
    # the ray meets mesh 1 (x = +1) first and the two in turn: hit k is on mesh (k + 1) % 2, and the tag is that + 2 * (1 + 1)
    assert records["mesh"][0] == (bounces + 1) % 2 + 4 and records["triangle"][0] // 2 == (bounces + 1) % 2
    assert status[1] == 0 and records["hit"][1] == 0 and records[1].tobytes() == bytes(48)
    same_records(records, want["records"], "facing mirrors, %d bounces" % bounces)
    assert np.array_equal(status, want["status"]) and last.view(np.uint32).tobytes() == want["last_rays"].view(np.uint32).tobytes()


# ---- 5. invalid arguments
def test_invalid_arguments_touch_nothing(pkg, hw11):
    import torch
    tracer, L = hw11["tracer"], pkg.lib()
    n = 64
    rays = np.array(hw11["rays"][:n])
    hits, status, last = np.full(48 * n, 0xEE, np.uint8), np.full(n, 0xEE, np.uint8), np.full(24 * n, 0xEE, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    o = pkg.make_options(0)
    gi = pkg.make_options(0, use_gi=True)
    INVALID = 1
    assert L.crt_guide_rays(tracer.ctx, p(rays), n, 0, C.byref(o), 64, p(hits), p(status), p(last)) == INVALID
    assert L.crt_guide_rays(tracer.ctx, None, n, 0, C.byref(o), 4, p(hits), p(status), p(last)) == INVALID
    assert L.crt_guide_rays(tracer.ctx, p(rays), n, 0, None, 4, p(hits), p(status), p(last)) == INVALID
    assert L.crt_guide_rays(tracer.ctx, p(rays), n, 0, C.byref(o), 4, None, p(status), p(last)) == INVALID
    assert L.crt_guide_rays(tracer.ctx, p(rays), n, 4, C.byref(o), 4, p(hits), p(status), p(last)) == INVALID
    assert np.all(hits == 0xEE) and np.all(status == 0xEE) and np.all(last == 0xEE)
    d_rays = torch.from_numpy(rays).cuda()
    d_hits = torch.full((48 * n,), 0xEE, dtype=torch.uint8, device="cuda")
    d_status = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    work = torch.full((tracer.guide_work_bytes(n) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    assert tracer.guide_work_bytes(n) == 512 + 120 * n and work.data_ptr() % 16 == 0
    for d_work in (None, work.data_ptr() + 4):
        rc = L.crt_guide_rays_device(tracer.ctx, C.c_void_p(d_rays.data_ptr()), n, 0, C.byref(o), 4, C.c_void_p(d_hits.data_ptr()),
                                     C.c_void_p(d_status.data_ptr()), None, C.c_void_p(d_work) if d_work else None, None)
        assert rc == INVALID
    torch.cuda.synchronize()
    assert bool(torch.all(d_hits == 0xEE)) and bool(torch.all(d_status == 0xEE)) and bool(torch.all(work == 0xEE))
    # use_gi left set is fine and ignored
    want = tracer.guide_rays(rays, pkg.RAY_PRIMARY, 4)
    assert L.crt_guide_rays(tracer.ctx, p(rays), n, 0, C.byref(gi), 4, p(hits), p(status), p(last)) == 0
    assert hits.tobytes() == want[0].tobytes() and np.array_equal(status, want[1])
    # the device call gives the host call's bits, and writes no byte beyond its work area
    tracer.guide_rays_device(d_rays.data_ptr(), n, pkg.RAY_PRIMARY, 4, d_hits.data_ptr(), work.data_ptr(), d_status_ptr=d_status.data_ptr())
    torch.cuda.synchronize()
    assert d_hits.cpu().numpy().tobytes() == want[0].tobytes() and np.array_equal(d_status.cpu().numpy(), want[1])
    assert bool(torch.all(work[tracer.guide_work_bytes(n):] == 0xEE))
    with pytest.raises(pkg.CrtError):
        tracer.set_guide_bounces(64)
    assert tracer.guide_bounces() == 0


# ---- 6. the frame calls
def frames_of(pkg, tracer, split):
    a, d, t = adaptive_settings(pkg, 4, 4), pkg.make_denoise(), pkg.make_temporal()
    tracer.history_reset()
    tracer.render_adaptive(ps.frame_options(pkg, 3, 2, 1), a, split=split)
    den = tracer.render_denoised(d, split=split)
    acc, valid = tracer.render_accumulated(t, d, valid=True, split=split)
    return den, acc, valid, tracer.history_frames(split=split)


@pytest.mark.parametrize("split", [False, True])
def test_zero_guide_bounces_change_nothing(pkg, scenes, hw11, split):
    tracer = hw11["tracer"]
    fresh = pkg.Tracer(pkg.Scene(json_text=scenes.to_json(hw11["scene"])))
    want = frames_of(pkg, fresh, split)
    try:
        tracer.set_guide_bounces(4)
        with_guides = frames_of(pkg, tracer, split)
        tracer.set_guide_bounces(0)
        got = frames_of(pkg, tracer, split)
    finally:
        tracer.set_guide_bounces(0)
    for a, b in zip(got[:3], want[:3]):
        assert a.tobytes() == b.tobytes()
    assert got[3] == want[3] == with_guides[3] == 1
    assert np.array_equal(with_guides[2], want[2]), "out_valid: the temporal stage keeps the first-hit guides"
    assert with_guides[0].tobytes() != want[0].tobytes()


def test_the_denoised_frame_is_the_rule_under_the_chain_guides(pkg, hw11):
    tracer = hw11["tracer"]
    colours = sample_colours(pkg, tracer, "hw11", 3, 2)[:4]
    state = ads.run(colours, (4, 4, 0.05, 1e-4))
    mean, var = dns.variance(state["total"], state["sq"], state["counts"])
    chain = tracer.guide_rays(hw11["rays"], pkg.RAY_PRIMARY, 4)[0]
    want = dns.denoise(mean, var, chain, H, W, dns.DEFAULTS)[0]
    try:
        tracer.set_guide_bounces(4)
        assert tracer.guide_bounces() == 4
        tracer.render_adaptive(ps.frame_options(pkg, 3, 2, 1), adaptive_settings(pkg, 4, 4))
        got = tracer.render_denoised(pkg.make_denoise())
        serial_frames = tracer.history_frames()
        tracer.set_guide_bounces(2)          # drops the kept guides alone
        other = tracer.render_denoised(pkg.make_denoise())
        assert tracer.history_frames() == serial_frames
    finally:
        tracer.set_guide_bounces(0)
    dns.same(got.reshape(-1), np.asarray(want).reshape(-1), "crt_render_denoised under 4-bounce chain guides")
    want2 = dns.denoise(mean, var, tracer.guide_rays(hw11["rays"], pkg.RAY_PRIMARY, 2)[0], H, W, dns.DEFAULTS)[0]
    dns.same(other.reshape(-1), np.asarray(want2).reshape(-1), "... under 2-bounce chain guides")


# ---- 7. it keeps what the mirror shows
def test_it_keeps_what_the_mirror_shows(pkg, scenes, oracle):
    """the hw11 room with a mirror on the back wall, depth 3, 2 GI samples, 4 samples a pixel, against the oracle's 64-sample frame, over
    the pixels whose first hit is the mirror and whose chain ends on a diffuse mesh.  The restatements on the CPU (tests/test_guides_host.py):
    the mean 0.03592, first-hit guides A 0.04117, chain guides B 0.03285, B / A 0.798 over 296 pixels."""
    m = restated_measure(scenes, oracle)
    where, truth = m["where"], m["truth"]
    noisy, a, b = m["rmse"]
    assert where.sum() >= 150
    tracer = tracer_of(pkg, scenes, "wall")
    d = pkg.make_denoise()
    try:
        tracer.set_guide_bounces(0)
        _, counts = tracer.render_adaptive(ps.frame_options(pkg, g.FRAME["depth"], g.FRAME["gi_samples"], 1), adaptive_settings(pkg, 4, 4))
        assert np.all(counts == 4)
        first = tracer.render_denoised(d)
        tracer.set_guide_bounces(4)
        chain = tracer.render_denoised(d)
    finally:
        tracer.set_guide_bounces(0)
    got_a, got_b = dns.rmse(first, truth, where), dns.rmse(chain, truth, where)
    print("restatement: the mean %.5f, A %.5f, B %.5f, B / A %.4f; the library's frames: A %.5f, B %.5f, ratio %.4f over %d pixels"
          % (noisy, a, b, b / a, got_a, got_b, got_b / got_a, int(where.sum())))
    assert b < a
    assert got_b < got_a and abs(got_b / got_a - b / a) <= 0.1 * (b / a)


# ---- 8. graph capture and replay; a capture refuses what it cannot do
def test_graph_capture_and_replay(pkg, scenes, hw11):
    import torch
    tracer = pkg.Tracer(pkg.Scene(json_text=scenes.to_json(hw11["scene"])))   # a context of its own: no other test's scratch
    n = PIXELS
    sets = [np.array(hw11["rays"]), np.array(hw11["rays"][::-1])]
    wants = [tracer.guide_rays(s, pkg.RAY_PRIMARY, 8) for s in sets]
    assert wants[0][0].tobytes() != wants[1][0].tobytes()
    d_rays = torch.from_numpy(sets[0]).cuda()
    d_hits = torch.zeros((n, 48), dtype=torch.uint8, device="cuda")
    d_status = torch.zeros((n,), dtype=torch.uint8, device="cuda")
    d_last = torch.zeros((n, 6), dtype=torch.float32, device="cuda")
    work = torch.zeros((tracer.guide_work_bytes(n),), dtype=torch.uint8, device="cuda")
    call = lambda stream: tracer.guide_rays_device(d_rays.data_ptr(), n, pkg.RAY_PRIMARY, 8, d_hits.data_ptr(), work.data_ptr(), d_status_ptr=d_status.data_ptr(),
                                                   d_last_rays_ptr=d_last.data_ptr(), stream_ptr=stream)
    # an open call would have to be harvested: refused before anything is enqueued, and the capture stays valid
    call(None)
    torch.cuda.synchronize()
    d_hits.zero_()
    x = torch.zeros(8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = x + 1
        with pytest.raises(pkg.CrtError) as e:
            call(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert e.value.code == pkg.CRT_ERR_INVALID and "open call" in str(e.value) and "captured" in str(e.value), str(e.value)
    graph.replay()
    torch.cuda.synchronize()
    assert y.cpu().tolist() == [1.0] * 8 and not bool(d_hits.any()), "a refused call enqueues nothing"
    del graph
    # harvested: the same call is captured, and two replays give the host variant's bits for two ray sets
    tracer.query_stats()
    generation = tracer.query_scratch_generation()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for s, want in zip(sets, wants):
        d_rays.copy_(torch.from_numpy(s))
        d_hits.zero_(); d_status.zero_(); d_last.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert d_hits.cpu().numpy().tobytes() == want[0].tobytes() and np.array_equal(d_status.cpu().numpy(), want[1])
        assert d_last.cpu().numpy().view(np.uint32).tobytes() == want[2].view(np.uint32).tobytes()
    assert tracer.query_scratch_generation() == generation
    del graph


# ---- 9. the host variant in several round trips: the same records, and statistics of the whole call
def test_the_host_variant_in_chunks(pkg, hw11):
    tracer, rays = hw11["tracer"], hw11["rays"]
    want = tracer.guide_rays(rays, pkg.RAY_PRIMARY, 8)
    whole = tracer.query_stats()
    try:
        tracer.set_query_chunks(host_rays=500, launch_rays=192)
        got = tracer.guide_rays(rays, pkg.RAY_PRIMARY, 8)
        chunked = tracer.query_stats()
    finally:
        tracer.set_query_chunks()
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
    assert (chunked.rays, chunked.hits) == (whole.rays, whole.hits) == (PIXELS, whole.hits) and whole.hits >= PIXELS


# ---- 10. the C++ host layer's drivers
def test_the_drivers_take_guide_bounces(pkg, scenes, tmp_path):
    import os
    import subprocess
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "course-assignment-danielhalachev_amd")
    main, animation = os.path.join(root, "crt_main"), os.path.join(root, "crt_animation")
    assert os.path.exists(main) and os.path.exists(animation), "the drivers are not built"
    scene = scenes.make("hw11", width=64, height=40, detail=0.2)
    scene["settings"]["image_settings"]["bucket_size"] = 16
    (tmp_path / "scene.crtscene").write_text(scenes.to_json(scene))
    gi = ["--depth", "2", "--gi", "2", "1", "--seed", "41", "--adaptive", "0.1", "2", "4", "--denoise", "2"]
    for tag, extra in (("plain", []), ("zero", ["--guide-bounces", "0"]), ("chain", ["--guide-bounces", "4"])):
        r = subprocess.run([main, "scene.crtscene", tag + ".ppm", *gi, *extra], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr
    read = lambda tag: (tmp_path / (tag + ".ppm")).read_bytes()
    assert read("plain") == read("zero") and read("chain") != read("plain")
    for bad in (["--gi", "2", "1", "--adaptive", "0.1", "2", "4", "--guide-bounces", "4"], [*gi, "--guide-bounces", "64"]):
        r = subprocess.run([main, "scene.crtscene", "no.ppm", *bad], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
        assert r.returncode != 0 and "usage:" in r.stderr and not (tmp_path / "no.ppm").exists()
    orbit = ["--depth", "2", "--fps", "2", "--seconds", "1", "--gi", "2", "--seed", "41", "--adaptive", "0.1", "2", "4", "--denoise", "2", "--temporal"]
    for tag, extra in (("a", []), ("b", ["--guide-bounces", "4"])):
        r = subprocess.run([animation, "scene.crtscene", tag + "_", *orbit, *extra], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr
    assert (tmp_path / "a_1.000000.ppm").read_bytes() != (tmp_path / "b_1.000000.ppm").read_bytes()
    r = subprocess.run([animation, "scene.crtscene", "no_", "--depth", "2", "--fps", "2", "--seconds", "1", "--guide-bounces", "4"], capture_output=True,
                       text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode != 0 and "usage:" in r.stderr and not (tmp_path / "no_0.000000.ppm").exists()
