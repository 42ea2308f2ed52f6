"""Direct lighting for the caller's records on the GPU (include/crt_hip.h: crt_shade_hits*, crt_light_points*) against the CPU oracle:
the colour of a ray's record is OracleScene.shoot(origin, direction, RAY_REFLECTION, depth=0, max_depth=0), float for float (NaN
equals NaN) -- and, through crt_query_stats::rerouted, WHICH walk lit a record: the filter kernel, or the reference-order walk
behind it.  Only rays whose direction shoot_ray's normalisation leaves alone are used (tests/shade_sets.py)."""
import ctypes as C

import numpy as np
import pytest

import query_sets as qs
import shade_sets as ss
from helpers import assert_same_floats, assert_shaded, make, small_case

pytestmark = pytest.mark.gpu
_CASES = {}


def case(pkg, scenes, oracle, name, tmp_path_factory):
    """A scene's tracer, oracle, the fixed-point random rays, their records (crt_trace_rays) and the oracle's colours: made once."""
    if name not in _CASES:
        scene, depth, folder = small_case(scenes, name, tmp_path_factory.mktemp(name))
        tracer, o = make(pkg, scenes, oracle, scene, folder)
        rays = ss.fixed_point_rays(qs.random_rays())
        hits = tracer.trace_rays(rays, qs.RAY_REFLECTION)
        want_hits = qs.oracle_hits(o, scene, rays, qs.RAY_REFLECTION, pkg.HIT_DTYPE)
        assert np.array_equal(hits["hit"], want_hits["hit"]) and np.array_equal(hits["mesh"], want_hits["mesh"])
        status = ss.expected_status(pkg, scene, want_hits)
        status.setflags(write=False)
        want = ss.oracle_colours(o, rays)
        want.setflags(write=False)
        hits.setflags(write=False)
        _CASES[name] = dict(scene=scene, depth=depth, folder=folder, tracer=tracer, oracle=o, rays=rays, hits=hits, status=status, want=want)
    return _CASES[name]


# ---- 1. random rays
@pytest.mark.parametrize("name", ["hw08", "hw11", "hw12", "hw14"])
def test_random_rays_match_the_oracle(pkg, scenes, oracle, name, tmp_path_factory):
    c = case(pkg, scenes, oracle, name, tmp_path_factory)
    rgb, status = c["tracer"].shade_hits(c["hits"])
    st = c["tracer"].query_stats()
    n_diffuse = int((c["status"] == pkg.SHADE_DIFFUSE).sum())
    occ = ss.lights_occluded(c["oracle"], c["scene"], c["hits"][c["status"] == pkg.SHADE_DIFFUSE])
    partly = int(((occ.sum(axis=1) > 0) & (occ.sum(axis=1) < occ.shape[1])).sum())
    print("%s: records %d diffuse %d (partly shadowed %d) recurse %d background %d rerouted %d kernel %.3f ms" % (
        name, st.rays, st.hits, partly, int((status == pkg.SHADE_RECURSES).sum()), int((status == pkg.SHADE_BACKGROUND).sum()), st.rerouted, st.kernel_ms))
    assert n_diffuse >= 1200 and partly >= 300, "the set must not be an empty case"
    assert_shaded(pkg, rgb, status, c["status"], c["want"], name)
    assert np.any(c["want"][c["status"] == pkg.SHADE_DIFFUSE] > 0)
    assert (st.rays, st.hits) == (len(c["hits"]), n_diffuse)
    bg = np.asarray(c["scene"]["settings"]["background_color"], dtype=np.float32)
    assert_same_floats(rgb[status == pkg.SHADE_BACKGROUND], np.broadcast_to(bg, (int((status == pkg.SHADE_BACKGROUND).sum()), 3)), name + ": background")


# ---- 2. a constant material is the background
def test_constant_material_is_the_background(pkg, scenes, oracle, tmp_path_factory):
    c = case(pkg, scenes, oracle, "hw11", tmp_path_factory)
    scene = ss.with_material_type(c["scene"], 2, "constant")   # the back wall
    tracer, o = make(pkg, scenes, oracle, scene)
    hits = tracer.trace_rays(c["rays"], qs.RAY_REFLECTION)
    on_wall = (hits["hit"] != 0) & (np.array([ob["material_index"] for ob in scene["objects"]])[hits["mesh"]] == 2)
    assert int(on_wall.sum()) >= 100
    rgb, status = tracer.shade_hits(hits)
    want_status = ss.expected_status(pkg, scene, hits)
    assert np.all(want_status[on_wall] == pkg.SHADE_BACKGROUND)
    assert_shaded(pkg, rgb, status, want_status, ss.oracle_colours(o, c["rays"]), "constant back wall")
    bg = np.asarray(scene["settings"]["background_color"], dtype=np.float32)
    assert_same_floats(rgb[on_wall], np.broadcast_to(bg, (int(on_wall.sum()), 3)), "constant back wall: background")
    assert tracer.query_stats().hits == int((want_status == pkg.SHADE_DIFFUSE).sum())


# ---- 3. the reroute door: records at no finite point
def test_records_at_non_finite_points_are_rerouted_alone(pkg, scenes, oracle, tmp_path_factory):
    c = case(pkg, scenes, oracle, "hw11", tmp_path_factory)
    tracer, o, scene = c["tracer"], c["oracle"], c["scene"]
    rays = ss.fixed_point_rays(qs.in_plane_rays(scene))
    want_hits = qs.oracle_hits(o, scene, rays, qs.RAY_REFLECTION, pkg.HIT_DTYPE)
    want_status = ss.expected_status(pkg, scene, want_hits)
    expected = int(((want_status == pkg.SHADE_DIFFUSE) & ~np.isfinite(want_hits["point"]).all(axis=1)).sum())
    assert expected > 0
    hits = tracer.trace_rays(rays, qs.RAY_REFLECTION)
    rgb, status = tracer.shade_hits(hits)
    st = tracer.query_stats()
    print("in-plane: records %d diffuse %d at a non-finite point %d rerouted %d" % (st.rays, st.hits, expected, st.rerouted))
    assert st.rerouted >= expected
    assert st.rerouted < int((want_status == pkg.SHADE_DIFFUSE).sum()), "only the records the filter cannot take are rerouted"
    assert_shaded(pkg, rgb, status, want_status, ss.oracle_colours(o, rays), "in-plane")


# ---- 4. without the filter
def test_without_the_filter_every_diffuse_record_is_rerouted(pkg, scenes, oracle, tmp_path_factory):
    c = case(pkg, scenes, oracle, "hw11", tmp_path_factory)
    tracer, _ = make(pkg, scenes, oracle, c["scene"], tuning=dict(bvh=0))
    rgb, status = tracer.shade_hits(c["hits"])
    st = tracer.query_stats()
    n_diffuse = int((c["status"] == pkg.SHADE_DIFFUSE).sum())
    assert (st.rays, st.hits, st.rerouted) == (len(c["hits"]), n_diffuse, n_diffuse)
    assert_shaded(pkg, rgb, status, c["status"], c["want"], "bvh=0")


# ---- 5. launch shapes
def test_launch_shapes(pkg, scenes, oracle, tmp_path_factory):
    c = case(pkg, scenes, oracle, "hw11", tmp_path_factory)
    chunk = max(64, (pkg.make_tuning().fetch_chunk >> 16) & ~63)   # what a wave of the launch claims per atomic (crt_query.hip)
    for n in sorted({1, 63, 65, chunk + 1}):
        rgb, status = c["tracer"].shade_hits(c["hits"][:n])
        assert rgb.shape == (n, 3) and status.shape == (n,)
        assert_shaded(pkg, rgb, status, c["status"][:n], c["want"][:n], "first %d records" % n)
        st = c["tracer"].query_stats()
        assert (st.rays, st.hits) == (n, int((c["status"][:n] == pkg.SHADE_DIFFUSE).sum()))


# ---- 6. lights
@pytest.mark.parametrize("n_lights", [0, 1])
def test_lights(pkg, scenes, oracle, n_lights, tmp_path_factory):
    c = case(pkg, scenes, oracle, "hw08", tmp_path_factory)
    scene = ss.with_lights(c["scene"], c["scene"]["lights"][:n_lights])
    tracer, o = make(pkg, scenes, oracle, scene)
    rgb, status = tracer.shade_hits(c["hits"])          # (the geometry is the same: so are the records)
    want = ss.oracle_colours(o, c["rays"])
    assert_shaded(pkg, rgb, status, c["status"], want, "%d lights" % n_lights)
    diffuse = c["status"] == pkg.SHADE_DIFFUSE
    if n_lights == 0:
        assert np.all(rgb[diffuse].view(np.uint32) == 0)
        assert np.all(tracer.light_points(c["hits"]["point"][diffuse], c["hits"]["normal"][diffuse]).view(np.uint32) == 0)
    else:
        assert np.any(rgb[diffuse] > 0) and np.any(np.all(rgb[diffuse] == 0, axis=1)), "lit and unlit records"


# ---- 7. light_points
@pytest.mark.parametrize("name", ["hw08", "hw11"])
def test_light_points_is_a_white_surface(pkg, scenes, oracle, name, tmp_path_factory):
    c = case(pkg, scenes, oracle, name, tmp_path_factory)
    white = ss.white_scene(c["scene"])
    o = oracle.OracleScene(scenes.to_blob(white))
    diffuse = c["status"] == pkg.SHADE_DIFFUSE
    want = ss.oracle_colours(o, c["rays"][diffuse])
    assert_same_floats(want[:, 1], want[:, 0], "the oracle's green")
    assert_same_floats(want[:, 2], want[:, 0], "the oracle's blue")
    points, normals = c["hits"]["point"][diffuse].copy(), c["hits"]["normal"][diffuse].copy()
    tracer = c["tracer"]                               # (the scene's own tracer: the albedo plays no part)
    got = tracer.light_points(points, normals)
    st = tracer.query_stats()
    assert got.shape == (len(points),) and (st.rays, st.hits) == (len(points), len(points))
    assert_same_floats(got, want[:, 0], name + ": light_points")
    assert np.any(got > 0)
    # one point exactly at a light, one with a NaN coordinate: both leave the filter, nothing else changes
    light = np.asarray(c["scene"]["lights"][0]["position"], dtype=np.float32)
    k = len(points) // 2
    points2 = np.concatenate([points[:k], light[None, :], np.array([[0.5, np.nan, -2.0]], dtype=np.float32), points[k:]])
    normals2 = np.concatenate([normals[:k], np.array([[0, 1, 0], [0, 1, 0]], dtype=np.float32), normals[k:]])
    got2 = tracer.light_points(points2, normals2)
    st2 = tracer.query_stats()
    print("%s: points %d rerouted %d, with the two extras %d" % (name, len(points), st.rerouted, st2.rerouted))
    assert st2.rerouted == st.rerouted + 2 and (st2.rays, st2.hits) == (len(points) + 2, len(points) + 2)
    assert_same_floats(np.concatenate([got2[:k], got2[k + 2:]]), got, name + ": the other points")


# ---- 8. records that point nowhere
def test_invalid_records(pkg, scenes, oracle, tmp_path_factory):
    c = case(pkg, scenes, oracle, "hw11", tmp_path_factory)
    tracer = c["tracer"]
    desc = tracer.scene.desc
    hits = c["hits"][:300].copy()
    valid = np.flatnonzero(hits["hit"] != 0)
    a, b, d, e = valid[3], valid[40], valid[41], valid[120]
    hits["mesh"][a] = desc.n_meshes
    hits["triangle"][b] = desc.n_triangles
    hits["mesh"][d], hits["triangle"][d] = 0xFFFFFFFF, 0xFFFFFFFF
    miss = np.flatnonzero(hits["hit"] == 0)[0]
    hits["mesh"][miss], hits["triangle"][miss] = 0xFFFFFFFF, 0xFFFFFFFF   # hit == 0: nothing else of the record is looked at
    hits["hit"][e] = 7                                                    # any non-zero value is a hit
    rgb, status = tracer.shade_hits(hits)
    want_status = c["status"][:300].copy()
    want_status[[a, b, d]] = pkg.SHADE_INVALID
    assert_shaded(pkg, rgb, status, want_status, c["want"][:300], "invalid records among valid ones")
    assert np.all(rgb[[a, b, d]].view(np.uint32) == 0)


# ---- 9. the device variants, on a stream of their own; nothing else changes
def test_device_variants_on_a_stream_of_their_own(pkg, scenes, oracle, tmp_path_factory):
    import torch
    c = case(pkg, scenes, oracle, "hw11", tmp_path_factory)
    tracer, depth = c["tracer"], c["depth"]
    rgb0 = tracer.render(max_depth=depth).copy()
    want_rgb, _ = c["oracle"].render(depth)
    assert_same_floats(rgb0, want_rgb, "frame before")
    s0 = tracer.stats()
    host_rgb, host_status = tracer.shade_hits(c["hits"])
    diffuse = c["status"] == pkg.SHADE_DIFFUSE
    host_light = tracer.light_points(c["hits"]["point"][diffuse], c["hits"]["normal"][diffuse])
    n, m = len(c["hits"]), int(diffuse.sum())
    d_hits = torch.from_numpy(np.ascontiguousarray(c["hits"]).view(np.uint8).reshape(n, 48).copy()).cuda()
    d_rgb = torch.full((n + 1, 3), float("nan"), dtype=torch.float32, device="cuda")     # (one record more: must stay untouched)
    d_status = torch.full((n + 1,), 0xA5, dtype=torch.uint8, device="cuda")
    d_points = torch.from_numpy(c["hits"]["point"][diffuse].copy()).cuda()
    d_normals = torch.from_numpy(c["hits"]["normal"][diffuse].copy()).cuda()
    d_light = torch.full((m + 1,), float("nan"), dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        tracer.shade_hits_device(d_hits.data_ptr(), n, d_rgb.data_ptr(), d_status.data_ptr(), stream_ptr=stream.cuda_stream)
        st = tracer.query_stats()
        assert (st.rays, st.hits) == (n, m)
        tracer.light_points_device(d_points.data_ptr(), d_normals.data_ptr(), m, d_light.data_ptr(), stream_ptr=stream.cuda_stream)
        st = tracer.query_stats()
        assert (st.rays, st.hits) == (m, m)
        # without a status array
        d_rgb2 = torch.full((n, 3), float("nan"), dtype=torch.float32, device="cuda")
        tracer.shade_hits_device(d_hits.data_ptr(), n, d_rgb2.data_ptr(), None, stream_ptr=stream.cuda_stream)
    stream.synchronize()
    rgb, status, light = d_rgb.cpu().numpy(), d_status.cpu().numpy(), d_light.cpu().numpy()
    assert np.all(np.isnan(rgb[n:])) and status[n] == 0xA5 and np.isnan(light[m]), "written past the end"
    assert_same_floats(rgb[:n], host_rgb, "device colours")
    assert_same_floats(d_rgb2.cpu().numpy(), host_rgb, "device colours, no status")
    assert np.array_equal(status[:n], host_status)
    assert_same_floats(light[:m], host_light, "device light sums")
    assert_shaded(pkg, rgb[:n], status[:n], c["status"], c["want"], "device variant")
    s1 = tracer.stats()
    assert bytes(s1) == bytes(s0), "crt_stats changed"
    assert_same_floats(tracer.render(max_depth=depth), rgb0, "frame after")
    # behind a pending frame: waits for it, answers, and the frame is the same frame
    frame = np.zeros_like(rgb0)
    tracer.render_async(pkg.make_options(depth), rgb=frame)
    again, _ = tracer.shade_hits(c["hits"])
    tracer.wait()
    assert_same_floats(again, host_rgb, "behind a pending frame")
    assert_same_floats(frame, rgb0, "the pending frame")
    s2 = tracer.stats()
    assert (s2.fallback_frames, s2.queue_regrows, s2.queue_bytes) == (s0.fallback_frames, s0.queue_regrows, s0.queue_bytes)


# ---- 10. errors and refusals
def test_bad_arguments_are_errors_and_the_context_lives_on(pkg, scenes, oracle, tmp_path_factory):
    c = case(pkg, scenes, oracle, "hw11", tmp_path_factory)
    tracer, L = c["tracer"], pkg.lib()
    hits = np.ascontiguousarray(c["hits"][:64])
    rgb, status = np.zeros((64, 3), dtype=np.float32), np.zeros(64, dtype=np.uint8)
    pts, out = np.zeros((64, 3), dtype=np.float32), np.full(64, 5.0, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    opt, gi = pkg.make_options(0), pkg.make_options(0, use_gi=True)
    bad = [lambda: L.crt_shade_hits(tracer.ctx, None, 64, C.byref(opt), p(rgb), p(status)),
           lambda: L.crt_shade_hits(tracer.ctx, p(hits), 64, C.byref(opt), None, p(status)),
           lambda: L.crt_shade_hits(tracer.ctx, p(hits), 64, None, p(rgb), p(status)),
           lambda: L.crt_shade_hits(tracer.ctx, p(hits), 64, C.byref(gi), p(rgb), p(status)),
           lambda: L.crt_shade_hits_device(tracer.ctx, None, 64, C.byref(opt), None, None, None),
           lambda: L.crt_shade_hits_device(tracer.ctx, p(hits), 64, C.byref(gi), p(rgb), None, None),
           lambda: L.crt_light_points(tracer.ctx, None, p(pts), 64, 1e-4, p(out)),
           lambda: L.crt_light_points(tracer.ctx, p(pts), None, 64, 1e-4, p(out)),
           lambda: L.crt_light_points(tracer.ctx, p(pts), p(pts), 64, 1e-4, None),
           lambda: L.crt_light_points_device(tracer.ctx, p(pts), p(pts), 64, 1e-4, None, None)]
    for k, call in enumerate(bad):
        assert call() == pkg.CRT_ERR_INVALID, k
        assert L.crt_last_error(tracer.ctx), k
    assert L.crt_shade_hits(tracer.ctx, p(hits), 64, C.byref(gi), p(rgb), p(status)) == pkg.CRT_ERR_INVALID and b"use_gi" in L.crt_last_error(tracer.ctx)
    assert np.all(rgb == 0) and np.all(out == 5.0), "a refused call writes nothing"
    # n == 0 touches nothing, whatever else is passed
    assert L.crt_shade_hits(tracer.ctx, None, 0, None, None, None) == pkg.CRT_OK
    assert L.crt_shade_hits_device(tracer.ctx, None, 0, None, None, None, None) == pkg.CRT_OK
    assert L.crt_light_points(tracer.ctx, None, None, 0, 1e-4, None) == pkg.CRT_OK
    assert L.crt_light_points_device(tracer.ctx, None, None, 0, 1e-4, None, None) == pkg.CRT_OK
    r0, s0 = tracer.shade_hits(np.zeros(0, dtype=pkg.HIT_DTYPE))
    assert r0.shape == (0, 3) and s0.shape == (0,) and tracer.light_points(np.zeros((0, 3)), np.zeros((0, 3))).shape == (0,)
    with pytest.raises(ValueError):
        tracer.light_points(np.zeros((4, 3)), np.zeros((5, 3)))
    want_rgb, _ = c["oracle"].render(c["depth"])
    assert_same_floats(tracer.render(max_depth=c["depth"]), want_rgb, "frame after the errors")
    got, st = tracer.shade_hits(c["hits"])
    assert_shaded(pkg, got, st, c["status"], c["want"], "query after the errors")


def test_multi_device_tracer_refuses_shading(pkg, scenes):
    scene, _, _ = small_case(scenes, "hw07")
    tracer = pkg.Tracer(pkg.Scene(json_text=scenes.to_json(scene)), devices=[0, 0])
    with pytest.raises(RuntimeError, match="multi-device"):
        tracer.shade_hits(np.zeros(8, dtype=pkg.HIT_DTYPE))
    with pytest.raises(RuntimeError, match="multi-device"):
        tracer.light_points(np.zeros((8, 3)), np.ones((8, 3)))
    with pytest.raises(RuntimeError, match="multi-device"):
        tracer.shade_hits_device(0, 8, 0)
    with pytest.raises(RuntimeError, match="multi-device"):
        tracer.light_points_device(0, 0, 8, 0)
