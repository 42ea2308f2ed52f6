"""Ray queries on the GPU (include/crt_hip.h: crt_trace_rays*, crt_occluded_rays*, crt_camera_rays_device) against the CPU oracle's
per-ray entry points (OracleScene.trace / .occluded / .camera_ray): every float bit for bit (NaN equals NaN), every integer equal --
and, through crt_query_stats::rerouted, WHICH walk answered: the filter kernels, or the reference-order walk behind them."""
import os
import re
import subprocess

import numpy as np
import pytest

import query_sets as qs
from helpers import assert_same_floats, assert_same_hits, distances, small_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "course-assignment-danielhalachev_amd", "crt_main")
# oracle, on the CPU: hits of the 4096 random rays as REFLECTION rays, and how many are occluded within 3.0
RANDOM_HITS = {"hw08": 1505, "hw11": 2915, "hw14": 2914}
RANDOM_OCCLUDED_3 = {"hw08": 1077, "hw11": 2112, "hw14": 2216}
IN_PLANE_NON_FINITE = {"hw11": 404, "hw08": 276}


def setup(pkg, scenes, oracle, name, tmp_path, tuning=None):
    scene, depth, folder = small_case(scenes, name, tmp_path)
    tracer = pkg.Tracer(pkg.Scene(json_text=scenes.to_json(scene), folder=folder), tuning=pkg.make_tuning(**tuning) if tuning else None)
    return scene, depth, tracer, oracle.OracleScene(scenes.to_blob(scene))


def check_closest(pkg, tracer, o, scene, rays, ray_type, what, rerouted):
    want = qs.oracle_hits(o, scene, rays, ray_type, pkg.HIT_DTYPE)
    got = tracer.trace_rays(rays, ray_type)
    st = tracer.query_stats()
    print("%s: rays %d hits %d (oracle %d) rerouted %d (expected %s) non-finite winners %d kernel %.3f ms" % (
        what, st.rays, st.hits, int(want["hit"].sum()), st.rerouted, rerouted, qs.non_finite_winners(want), st.kernel_ms))
    assert_same_hits(got, want, what)
    assert st.rays == len(rays) and st.hits == int(want["hit"].sum())
    if rerouted == "non-finite winners":   # on the filter path exactly the rays whose miss the miss check refutes
        rerouted = qs.non_finite_winners(want)
    if rerouted is not None:
        assert st.rerouted == rerouted, what
    return want


def check_occluded(tracer, o, rays, dist, what, rerouted=None):
    want = qs.oracle_occluded(o, rays, dist)
    got = tracer.occluded_rays(rays, dist)
    st = tracer.query_stats()
    print("%s: rays %d occluded %d (oracle %d) rerouted %d" % (what, st.rays, st.hits, int(want.sum()), st.rerouted))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d rays differ, first %d" % (what, bad.size, bad[0])
    assert st.rays == len(rays) and st.hits == int(want.sum())
    if rerouted is not None:
        assert st.rerouted == rerouted, what
    return want


# ---- 1. random rays: the filter path answers
@pytest.mark.parametrize("ray_type", [qs.RAY_PRIMARY, qs.RAY_REFLECTION], ids=["primary", "reflection"])
@pytest.mark.parametrize("name", ["hw08", "hw11", "hw14", "hw12"])
def test_random_rays_match_the_oracle(pkg, scenes, oracle, name, ray_type, tmp_path):
    scene, _, tracer, o = setup(pkg, scenes, oracle, name, tmp_path)
    want = check_closest(pkg, tracer, o, scene, qs.random_rays(), ray_type, "%s type %d" % (name, ray_type), rerouted=0)
    assert qs.non_finite_winners(want) == 0
    if ray_type == qs.RAY_REFLECTION and name in RANDOM_HITS:
        assert int(want["hit"].sum()) == RANDOM_HITS[name]


# ---- 2. occlusion
@pytest.mark.parametrize("name", ["hw08", "hw11", "hw14", "hw12"])
def test_occlusion_matches_the_oracle(pkg, scenes, oracle, name, tmp_path):
    scene, _, tracer, o = setup(pkg, scenes, oracle, name, tmp_path)
    rays = qs.random_rays()
    want = check_occluded(tracer, o, rays, 3.0, name + " within 3.0", rerouted=0)
    if name in RANDOM_OCCLUDED_3:
        assert int(want.sum()) == RANDOM_OCCLUDED_3[name]
    check_occluded(tracer, o, rays, distances(len(rays)), name + " per-ray distances", rerouted=0)
    check_occluded(tracer, o, rays, np.float32(np.inf), name + " no limit")


# ---- 3. the refuted miss, by its own door
@pytest.mark.parametrize("ray_type", [qs.RAY_PRIMARY, qs.RAY_REFLECTION], ids=["primary", "reflection"])
@pytest.mark.parametrize("name", ["hw11", "hw08"])
def test_in_plane_rays_are_rerouted_ray_by_ray(pkg, scenes, oracle, name, ray_type, tmp_path):
    """A ray in a bounding plane of the scene: the filter finds no finite hit, the miss check finds a triangle the reference accepts
    at t = NaN / inf, and that ray alone goes to the reference-order walk: rerouted == the oracle's non-finite winners."""
    scene, _, tracer, o = setup(pkg, scenes, oracle, name, tmp_path)
    rays = qs.in_plane_rays(scene)
    want = qs.oracle_hits(o, scene, rays, ray_type, pkg.HIT_DTYPE)
    expected = qs.non_finite_winners(want)
    assert expected == (IN_PLANE_NON_FINITE[name] if ray_type == qs.RAY_REFLECTION else 0)
    check_closest(pkg, tracer, o, scene, rays, ray_type, "%s in-plane type %d" % (name, ray_type), rerouted=expected)
    # occlusion without a limit meets the same triangles (length = inf <= inf); with one, such a hit never occludes
    check_occluded(tracer, o, rays, np.float32(np.inf), name + " in-plane, no limit")
    check_occluded(tracer, o, rays, 3.0, name + " in-plane within 3.0", rerouted=0)


# ---- 4. rays the filter does not take
@pytest.mark.parametrize("scale", [0.5, 3.0, 1.0 + 2.0 ** -10])
def test_directions_not_of_unit_length_are_rerouted(pkg, scenes, oracle, scale, tmp_path):
    scene, _, tracer, o = setup(pkg, scenes, oracle, "hw11", tmp_path)
    rays = qs.random_rays()
    rays[:, 3:] *= np.float32(scale)
    check_closest(pkg, tracer, o, scene, rays, qs.RAY_REFLECTION, "scale %r" % scale, rerouted=len(rays))
    check_closest(pkg, tracer, o, scene, rays[:512], qs.RAY_PRIMARY, "scale %r primary" % scale, rerouted=512)
    check_occluded(tracer, o, rays, distances(len(rays)), "scale %r occlusion" % scale, rerouted=len(rays))


def test_non_finite_rays_are_rerouted(pkg, scenes, oracle, tmp_path):
    scene, _, tracer, o = setup(pkg, scenes, oracle, "hw11", tmp_path)
    rays = qs.random_rays(4)
    rays[0, 0] = np.inf
    rays[1, 1] = np.nan
    rays[2, 3] = np.inf
    rays[3, 5] = np.nan
    for ray_type in (qs.RAY_PRIMARY, qs.RAY_REFLECTION):
        check_closest(pkg, tracer, o, scene, rays, ray_type, "non-finite type %d" % ray_type, rerouted=4)
    check_occluded(tracer, o, rays, 3.0, "non-finite occlusion", rerouted=4)
    check_occluded(tracer, o, rays, np.float32(np.inf), "non-finite occlusion, no limit", rerouted=4)


def test_float32_unit_vectors_qualify(pkg, scenes, oracle, tmp_path):
    """Directions normalised in float32 (twice, like a frame's primary rays) and axis-aligned ones stay on the filter path."""
    scene, _, tracer, o = setup(pkg, scenes, oracle, "hw11", tmp_path)
    rays = qs.random_rays(1024, seed=21)
    d = rays[:, 3:] * np.float32(1.7)
    for _ in range(2):
        d = (d / np.sqrt((d * d).sum(axis=1, dtype=np.float32), dtype=np.float32)[:, None]).astype(np.float32)
    rays[:, 3:] = d
    rays[:6, 3:] = np.concatenate([np.eye(3), -np.eye(3)]).astype(np.float32)
    rays[:6, :3] = [0.3, 0.2, -3.1]
    check_closest(pkg, tracer, o, scene, rays, qs.RAY_REFLECTION, "float32 unit vectors", rerouted="non-finite winners")


# ---- 5. without the filter
def test_without_the_filter_every_ray_is_rerouted(pkg, scenes, oracle, tmp_path):
    scene, _, tracer, o = setup(pkg, scenes, oracle, "hw11", tmp_path, tuning=dict(bvh=0))
    rays = qs.random_rays()
    for ray_type in (qs.RAY_PRIMARY, qs.RAY_REFLECTION):
        check_closest(pkg, tracer, o, scene, rays, ray_type, "bvh=0 type %d" % ray_type, rerouted=len(rays))
    check_occluded(tracer, o, rays, 3.0, "bvh=0 within 3.0", rerouted=len(rays))
    check_occluded(tracer, o, rays, distances(len(rays)), "bvh=0 per-ray distances", rerouted=len(rays))
    check_occluded(tracer, o, rays, np.float32(np.inf), "bvh=0 no limit", rerouted=len(rays))


# ---- 6. camera rays: a depth / id pass on torch tensors
@pytest.mark.parametrize("name,rotated", [("hw07", False), ("hw11", True)])
def test_camera_rays_and_their_hits(pkg, scenes, oracle, name, rotated, tmp_path):
    import torch
    scene, _, tracer, o = setup(pkg, scenes, oracle, name, tmp_path)
    if rotated:
        pos, mat = tracer.scene.camera()
        pos, mat = pkg.camera_apply(pos, mat, "pan", 17.0)
        pos, mat = pkg.camera_apply(pos, mat, "tilt", -8.0)
        pos, mat = pkg.camera_apply(pos, mat, "truck", [0.3, 0.1, -0.4])
        tracer.set_camera(pos, mat)
        o.set_camera(pos, mat)
    h, w = tracer.height, tracer.width
    d_rays = torch.full((h * w, 6), float("nan"), dtype=torch.float32, device="cuda")
    d_hits = torch.full((h * w, 48), 0xA5, dtype=torch.uint8, device="cuda")
    tracer.camera_rays_device(d_rays.data_ptr())
    tracer.trace_rays_device(d_rays.data_ptr(), h * w, qs.RAY_PRIMARY, d_hits.data_ptr())   # (same stream: ordered behind the rays)
    st = tracer.query_stats()
    rays = d_rays.cpu().numpy()
    want_rays = np.array([np.concatenate(o.camera_ray(r, c)) for r in range(h) for c in range(w)], dtype=np.float32)
    assert_same_floats(rays, want_rays, name + " camera rays")
    want = qs.oracle_hits(o, scene, want_rays, qs.RAY_PRIMARY, pkg.HIT_DTYPE)
    got = d_hits.cpu().numpy().view(pkg.HIT_DTYPE).reshape(-1)
    assert_same_hits(got, want, name + " camera-ray hits")
    assert st.rays == h * w and st.hits == int(want["hit"].sum()) and st.rerouted == qs.non_finite_winners(want) == 0


# ---- 7. the device variants: another stream, sizes around a wave, a million rays
def test_device_variants_on_a_stream_of_their_own(pkg, scenes, oracle, tmp_path):
    import torch
    scene, _, tracer, o = setup(pkg, scenes, oracle, "hw11", tmp_path)
    base = qs.random_rays()
    want = qs.oracle_hits(o, scene, base, qs.RAY_REFLECTION, pkg.HIT_DTYPE)
    dist = distances(len(base))
    want_occ = qs.oracle_occluded(o, base, dist)
    stream = torch.cuda.Stream()
    for n in (0, 1, 65, 1_000_003):
        idx = np.arange(n) % len(base)
        d_rays = torch.from_numpy(base[idx]).cuda() if n else torch.zeros((1, 6), dtype=torch.float32, device="cuda")
        d_dist = torch.from_numpy(dist[idx]).cuda() if n else torch.zeros(1, dtype=torch.float32, device="cuda")
        d_hits = torch.full((max(n, 1) + 1, 48), 0xA5, dtype=torch.uint8, device="cuda")   # (one record more: must stay untouched)
        d_occ = torch.full((max(n, 1) + 1,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            tracer.trace_rays_device(d_rays.data_ptr(), n, qs.RAY_REFLECTION, d_hits.data_ptr(), stream.cuda_stream)
            if n:
                st = tracer.query_stats()
                assert (st.rays, st.hits, st.rerouted) == (n, int(want["hit"][idx].sum()), 0)
            tracer.occluded_rays_device(d_rays.data_ptr(), d_dist.data_ptr(), n, d_occ.data_ptr(), stream.cuda_stream)
            if n:
                st = tracer.query_stats()
                assert (st.rays, st.hits, st.rerouted) == (n, int(want_occ[idx].sum()), 0)
        stream.synchronize()
        hits, occ = d_hits.cpu().numpy(), d_occ.cpu().numpy()
        assert np.all(hits[n:] == 0xA5) and np.all(occ[n:] == 0xA5), "n = %d: written past the end" % n
        if n:
            assert_same_hits(hits[:n].view(pkg.HIT_DTYPE).reshape(-1), want[idx], "n = %d" % n)
            assert np.array_equal(occ[:n].astype(bool), want_occ[idx]), "n = %d occlusion" % n
    assert tracer.trace_rays(np.zeros((0, 6), dtype=np.float32)).shape == (0,)
    assert tracer.occluded_rays(np.zeros((0, 6), dtype=np.float32), 1.0).shape == (0,)


# ---- 8. a query changes nothing else
def test_queries_leave_frames_and_statistics_alone(pkg, scenes, oracle, tmp_path):
    scene, depth, tracer, o = setup(pkg, scenes, oracle, "hw11", tmp_path)
    rgb0 = tracer.render(max_depth=depth).copy()
    want_rgb, _ = o.render(depth)
    assert_same_floats(rgb0, want_rgb, "frame before the queries")
    s0 = tracer.stats()
    rays, in_plane = qs.random_rays(), qs.in_plane_rays(scene)
    want = check_closest(pkg, tracer, o, scene, rays, qs.RAY_REFLECTION, "between frames", rerouted=0)
    check_closest(pkg, tracer, o, scene, in_plane, qs.RAY_REFLECTION, "between frames, in-plane", rerouted=IN_PLANE_NON_FINITE["hw11"])
    check_occluded(tracer, o, rays, 3.0, "between frames, occlusion", rerouted=0)
    s1 = tracer.stats()
    assert (s1.fallback_frames, s1.queue_regrows, s1.queue_bytes, s1.pixels) == (s0.fallback_frames, s0.queue_regrows, s0.queue_bytes, s0.pixels)
    assert_same_floats(tracer.render(max_depth=depth), rgb0, "frame after the queries")
    s2 = tracer.stats()
    assert (s2.fallback_frames, s2.queue_regrows, s2.queue_bytes) == (s0.fallback_frames, s0.queue_regrows, s0.queue_bytes)
    # a query while a frame is pending: it waits for the frame, answers, and the frame is the same frame
    rgb = np.zeros_like(rgb0)
    tracer.render_async(pkg.make_options(depth), rgb=rgb)
    got = tracer.trace_rays(rays, qs.RAY_REFLECTION)
    assert_same_hits(got, want, "query behind a pending frame")
    tracer.wait()
    assert_same_floats(rgb, rgb0, "the pending frame")
    s3 = tracer.stats()
    assert (s3.fallback_frames, s3.queue_regrows, s3.queue_bytes) == (s0.fallback_frames, s0.queue_regrows, s0.queue_bytes)


# ---- 9. errors
def test_bad_arguments_are_errors_and_the_context_lives_on(pkg, scenes, oracle, tmp_path):
    import ctypes as C
    scene, depth, tracer, o = setup(pkg, scenes, oracle, "hw11", tmp_path)
    L = pkg.lib()
    rays = qs.random_rays(64)
    hits = np.zeros(64, dtype=pkg.HIT_DTYPE)
    occ = np.zeros(64, dtype=np.uint8)
    dist = np.ones(64, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    bad = [lambda: L.crt_trace_rays(tracer.ctx, None, 64, 2, p(hits)), lambda: L.crt_trace_rays(tracer.ctx, p(rays), 64, 2, None),
           lambda: L.crt_trace_rays(tracer.ctx, p(rays), 64, 7, p(hits)), lambda: L.crt_trace_rays_device(tracer.ctx, None, 64, 2, None, None),
           lambda: L.crt_trace_rays_device(tracer.ctx, p(rays), 64, 7, p(hits), None),
           lambda: L.crt_occluded_rays(tracer.ctx, p(rays), None, 64, p(occ)), lambda: L.crt_occluded_rays(tracer.ctx, None, p(dist), 64, p(occ)),
           lambda: L.crt_occluded_rays_device(tracer.ctx, p(rays), p(dist), 64, None, None), lambda: L.crt_camera_rays_device(tracer.ctx, None, None)]
    for k, call in enumerate(bad):
        assert call() == pkg.CRT_ERR_INVALID, k
        assert L.crt_last_error(tracer.ctx), k
    assert L.crt_trace_rays(tracer.ctx, p(rays), 64, 7, p(hits)) == pkg.CRT_ERR_INVALID and b"ray_type" in L.crt_last_error(tracer.ctx)
    assert L.crt_trace_rays(tracer.ctx, None, 0, 7, None) == pkg.CRT_OK          # n == 0 touches nothing
    with pytest.raises(pkg.CrtError):
        tracer.trace_rays(rays, 7)
    want_rgb, _ = o.render(depth)
    assert_same_floats(tracer.render(max_depth=depth), want_rgb, "frame after the errors")
    check_closest(pkg, tracer, o, scene, rays, qs.RAY_REFLECTION, "query after the errors", rerouted=0)


def test_multi_device_tracer_refuses_queries(pkg, scenes):
    scene, _, _ = small_case(scenes, "hw07")
    tracer = pkg.Tracer(pkg.Scene(json_text=scenes.to_json(scene)), devices=[0, 0])
    with pytest.raises(RuntimeError, match="multi-device"):
        tracer.trace_rays(qs.random_rays(8))
    with pytest.raises(RuntimeError, match="multi-device"):
        tracer.occluded_rays(qs.random_rays(8), 1.0)


# ---- 10. picking from the command line
def test_crt_main_probe_prints_the_centre_pixels_hit(pkg, scenes, oracle, tmp_path):
    scene, _, _ = small_case(scenes, "hw07")
    (tmp_path / "scene.crtscene").write_text(scenes.to_json(scene))
    o = oracle.OracleScene(scenes.to_blob(scene))
    row, col = o.height // 2, o.width // 2
    r = subprocess.run([EXE, "scene.crtscene", "unused.ppm", "--probe", str(row), str(col)], capture_output=True, text=True, timeout=120,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    origin, direction = o.camera_ray(row, col)
    want = qs.oracle_hits(o, scene, np.concatenate([origin, direction])[None, :], qs.RAY_PRIMARY, pkg.HIT_DTYPE)[0]
    assert want["hit"] == 1, "the centre pixel of hw07 sees the scene"
    m = re.search(r"probe row (\d+) col (\d+): mesh (\d+) triangle (\d+) t (\S+) point (\S+) (\S+) (\S+) normal (\S+) (\S+) (\S+)", r.stdout)
    assert m, r.stdout
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4))) == (row, col, int(want["mesh"]), int(want["triangle"]))
    assert float.fromhex(m.group(5)) == float(want["t"])
    assert [float.fromhex(m.group(k)) for k in (6, 7, 8)] == [float(x) for x in want["point"]]
    assert [float.fromhex(m.group(k)) for k in (9, 10, 11)] == [float(x) for x in want["normal"]]
    assert not (tmp_path / "unused.ppm").exists()
