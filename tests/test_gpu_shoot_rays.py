"""Radiance queries on the GPU (include/crt_hip.h: crt_shoot_rays*) against the CPU oracle: the colour of a ray is
OracleScene.shoot(origin, direction, ray_type, depth=0, max_depth), float for float (NaN equals NaN), for directions as the caller has
them -- and against the library's own frame, which is the special case of the camera's rays shot as PRIMARY rays."""
import ctypes as C

import numpy as np
import pytest

import query_sets as qs
import shade_sets as ss
import shoot_sets as sh
from helpers import assert_same_floats, level_rays, make, small_case
from shoot_sets import case

pytestmark = pytest.mark.gpu
SCENES = ["hw08", "hw11", "hw12", "hw14"]


# ---- 1. random rays against the oracle
@pytest.mark.parametrize("name", SCENES)
def test_random_rays_match_the_oracle(pkg, scenes, oracle, name, tmp_path_factory):
    c = case(pkg, scenes, oracle, name, tmp_path_factory)
    tracer, rays, depth = c["tracer"], c["rays"], c["depth"]
    assert len(rays) >= 4096 and np.array_equal(rays[:4096], qs.random_rays())
    types = sh.first_hit_types(pkg, c["oracle"], c["scene"], rays)
    recursing = int(np.isin(types, sh.RECURSING).sum())
    rgb = tracer.shoot_rays(rays, qs.RAY_REFLECTION, max_depth=depth)
    st, qst = tracer.shoot_stats(), tracer.query_stats()
    lr = level_rays(st)
    print("%s: rays %d depth %d first hits recursing %d levels %d level_rays %s shadow_records %d rerouted %d kernel %.3f ms" % (
        name, st.rays, depth, recursing, st.levels, lr[:st.levels], st.shadow_records, st.rerouted, st.kernel_ms))
    if name in ("hw11", "hw14"):   # conditions on the input: the set must not be an empty case
        assert recursing >= 100 and lr[1] > 0
    if name == "hw14":
        assert lr[2] > 0
    assert rgb.shape == (len(rays), 3) and rgb.dtype == np.float32
    assert_same_floats(rgb, c["want"], name)
    assert st.rays == len(rays) == lr[0] and 1 <= st.levels <= depth + 1 and all(x == 0 for x in lr[st.levels:])
    assert (qst.rays, qst.hits, qst.rerouted) == (len(rays), int((types != "miss").sum()), st.rerouted)
    # level 1 holds a reflection ray for every recursing first hit, and at most one transmission ray more
    assert recursing <= lr[1] <= 2 * recursing
    assert st.shadow_records >= int((types == "diffuse").sum()) and st.kernel_ms > 0


# ---- 2. PRIMARY rays cull back faces
@pytest.mark.parametrize("name", ["hw11", "hw14"])
def test_primary_rays(pkg, scenes, oracle, name, tmp_path_factory):
    c = case(pkg, scenes, oracle, name, tmp_path_factory)
    rays = c["rays"][:1024]
    want = sh.oracle_colours(c["oracle"], rays, c["depth"], qs.RAY_PRIMARY)
    assert np.any(want.view(np.uint32) != c["want"][:1024].view(np.uint32)), "the ray type must matter for this set"
    assert_same_floats(c["tracer"].shoot_rays(rays, qs.RAY_PRIMARY, max_depth=c["depth"]), want, name + ": PRIMARY")


# ---- 3. the frame is a special case
def shoot_camera_rays(tracer, depth, **biases):
    import torch
    n = tracer.width * tracer.height
    d_rays = torch.zeros((n, 6), dtype=torch.float32, device="cuda")
    d_rgb = torch.full((n, 3), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    tracer.camera_rays_device(d_rays.data_ptr())
    tracer.shoot_rays_device(d_rays.data_ptr(), n, d_rgb.data_ptr(), qs.RAY_PRIMARY, max_depth=depth, **biases)
    torch.cuda.synchronize()
    return d_rgb.cpu().numpy().reshape(tracer.height, tracer.width, 3)


@pytest.mark.parametrize("bvh", [1, 0])
@pytest.mark.parametrize("name", SCENES)
def test_the_frame_is_a_special_case(pkg, scenes, oracle, name, bvh, tmp_path_factory):
    c = case(pkg, scenes, oracle, name, tmp_path_factory)
    depth = c["depth"]
    tracer = c["tracer"] if bvh else make(pkg, scenes, oracle, c["scene"], c["folder"], tuning=dict(bvh=0))[0]
    frame = tracer.render(max_depth=depth).copy()
    s0 = tracer.stats()
    got = shoot_camera_rays(tracer, depth)
    st = tracer.shoot_stats()
    print("%s bvh=%d: levels %d level_rays %s rerouted %d kernel %.3f ms" % (name, bvh, st.levels, level_rays(st)[:st.levels], st.rerouted, st.kernel_ms))
    assert_same_floats(got, frame, "%s bvh=%d: the camera's rays shot as PRIMARY rays are the frame" % (name, bvh))
    if not bvh:
        assert st.rerouted >= st.rays, "without the filter every ray is walked in the reference's order"
    if name == "hw14":
        biases = dict(shadow_bias=1e-3, reflection_bias=2e-3, refraction_bias=5e-4)
        biased = np.zeros_like(frame)
        tracer.render_async(pkg.make_options(depth, **biases), rgb=biased)
        tracer.wait()
        assert np.any(biased.view(np.uint32) != frame.view(np.uint32)), "the biases must matter for this frame"
        assert_same_floats(shoot_camera_rays(tracer, depth, **biases), biased, "%s bvh=%d: non-default biases" % (name, bvh))
    assert_same_floats(tracer.render(max_depth=depth), frame, "the frame rendered again")
    s1 = tracer.stats()
    assert (s1.fallback_frames, s1.queue_bytes, s1.queue_regrows) == (s0.fallback_frames, s0.queue_bytes, s0.queue_regrows)


# ---- 4. depth sweep
def test_depth_sweep(pkg, scenes, oracle, tmp_path_factory):
    c = case(pkg, scenes, oracle, "hw14", tmp_path_factory)
    tracer, o = c["tracer"], c["oracle"]
    rays = np.ascontiguousarray(sh.shaped_rays(c["scene"])[:512])
    for max_depth in range(c["depth"] + 1):
        rgb = tracer.shoot_rays(rays, max_depth=max_depth)
        st = tracer.shoot_stats()
        lr = level_rays(st)
        print("max_depth %d: levels %d level_rays %s" % (max_depth, st.levels, lr[:st.levels]))
        assert_same_floats(rgb, sh.oracle_colours(o, rays, max_depth), "max_depth %d" % max_depth)
        assert st.levels <= max_depth + 1 and lr[0] == 512
        assert all(lr[g + 1] <= 2 * lr[g] for g in range(63))
        if max_depth == 0:
            assert st.levels == 1
            walked = sh.normalized_rays(rays)
            assert_same_floats(walked[:, 3:], ss.normalized_like_shoot_ray(rays), "shoot_ray's normalisation")
            direct, status = tracer.shade_hits(tracer.trace_rays(walked, qs.RAY_REFLECTION))
            final = (status == pkg.SHADE_DIFFUSE) | (status == pkg.SHADE_BACKGROUND)
            assert int(final.sum()) > 100 and int((~final).sum()) > 100
            assert_same_floats(rgb[final], direct[final], "max_depth 0: diffuse and background rows are shade_hits(trace_rays(.))")
        if max_depth >= 2:
            assert lr[1] > 0 and lr[2] > 0


# ---- 5. launch shapes
def test_launch_shapes(pkg, scenes, oracle, tmp_path_factory):
    c = case(pkg, scenes, oracle, "hw14", tmp_path_factory)
    tracer, depth = c["tracer"], c["depth"]
    rays = sh.shaped_rays(c["scene"])
    assert rays.shape == (4096, 6)
    full = tracer.shoot_rays(rays, max_depth=depth)
    assert_same_floats(full, sh.oracle_colours(c["oracle"], rays, depth), "the full set")
    for n in (1, 63, 64, 65, 257, 4096):
        got = tracer.shoot_rays(rays[:n], max_depth=depth)
        st = tracer.shoot_stats()
        assert got.shape == (n, 3) and st.rays == n == level_rays(st)[0]
        assert_same_floats(got, full[:n], "first %d rays" % n)
        assert np.array_equal(tracer.shoot_rays(rays[:n], max_depth=depth).view(np.uint32), got.view(np.uint32)), "two identical calls, n = %d" % n


# ---- 6. directions as the caller has them
@pytest.mark.parametrize("scale", [0.5, 3.0, 1 + 2.0 ** -10])
def test_scaled_directions(pkg, scenes, oracle, scale, tmp_path_factory):
    c = case(pkg, scenes, oracle, "hw11", tmp_path_factory)
    rays = c["rays"].copy()
    rays[:, 3:] *= np.float32(scale)
    assert_same_floats(c["tracer"].shoot_rays(rays, max_depth=c["depth"]), sh.oracle_colours(c["oracle"], rays, c["depth"]), "directions x %r" % scale)


def test_in_plane_zero_and_nan_rays(pkg, scenes, oracle, tmp_path_factory):
    c = case(pkg, scenes, oracle, "hw11", tmp_path_factory)
    tracer, o, depth = c["tracer"], c["oracle"], c["depth"]
    rays = qs.in_plane_rays(c["scene"])
    want = sh.oracle_colours(o, rays, depth)
    assert int(np.isnan(want).any(axis=1).sum()) > 100, "records at t = inf / NaN colour some of these rays NaN"
    assert_same_floats(tracer.shoot_rays(rays, max_depth=depth), want, "in-plane rays")
    st = tracer.shoot_stats()
    print("in-plane: rays %d rerouted %d levels %d" % (st.rays, st.rerouted, st.levels))
    assert st.rerouted > 0
    odd = np.array([[0.0, 0.5, -2.0, 0.0, 0.0, 0.0], [np.nan, 0.5, -2.0, 0.0, 0.0, -1.0], [0.0, 0.5, 1.0, 0.0, 0.0, -2.0]], dtype=np.float32)
    assert_same_floats(tracer.shoot_rays(odd, max_depth=depth), sh.oracle_colours(o, odd, depth), "a zero direction, a NaN origin")
    assert tracer.shoot_stats().rerouted >= 2


# ---- 7. the device variant, on a stream of its own
def test_device_variant_on_a_stream_of_its_own(pkg, scenes, oracle, tmp_path_factory):
    import torch
    c = case(pkg, scenes, oracle, "hw14", tmp_path_factory)
    tracer, depth, rays = c["tracer"], c["depth"], c["rays"]
    n = len(rays)
    host = tracer.shoot_rays(rays, max_depth=depth)
    host_stats = tracer.shoot_stats()
    d_rays = torch.from_numpy(rays.copy()).cuda()
    d_rgb = torch.full((n + 1, 3), float("nan"), dtype=torch.float32, device="cuda")     # (one row more: must stay untouched)
    sentinel = torch.full((8, 3), 7.5, dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        tracer.shoot_rays_device(d_rays.data_ptr(), n, d_rgb.data_ptr(), max_depth=depth, stream_ptr=stream.cuda_stream)
        st = tracer.shoot_stats()
        tracer.shoot_rays_device(d_rays.data_ptr(), 0, sentinel.data_ptr(), max_depth=depth, stream_ptr=stream.cuda_stream)
        assert pkg.lib().crt_shoot_rays_device(tracer.ctx, None, 0, 7, None, None, None) == pkg.CRT_OK
    stream.synchronize()
    rgb = d_rgb.cpu().numpy()
    assert np.all(np.isnan(rgb[n:])), "written past the end"
    assert np.all(sentinel.cpu().numpy() == 7.5), "n == 0 touches nothing"
    assert_same_floats(rgb[:n], host, "device colours")
    assert_same_floats(rgb[:n], c["want"], "device colours against the oracle")
    assert (st.rays, st.levels, level_rays(st), st.shadow_records) == (host_stats.rays, host_stats.levels, level_rays(host_stats), host_stats.shadow_records)
    assert tracer.shoot_stats().rays == n, "a call with n == 0 leaves the statistics alone"
    # a ray query behind it on the default stream, and the radiance query again: both still right
    hits = tracer.trace_rays(sh.normalized_rays(rays[:256]), qs.RAY_REFLECTION)
    assert int((hits["hit"] != 0).sum()) == tracer.query_stats().hits
    assert_same_floats(tracer.shoot_rays(rays, max_depth=depth), host, "after a ray query")


# ---- 8. errors and refusals
def test_bad_arguments_are_errors_and_the_context_lives_on(pkg, scenes, oracle, tmp_path_factory):
    c = case(pkg, scenes, oracle, "hw11", tmp_path_factory)
    tracer, L = c["tracer"], pkg.lib()
    rays = np.ascontiguousarray(c["rays"][:64])
    rgb = np.full((64, 3), 5.0, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    opt, gi, deep = pkg.make_options(5), pkg.make_options(5, use_gi=True), pkg.make_options(64)
    bad = [(lambda: L.crt_shoot_rays(tracer.ctx, None, 64, 2, C.byref(opt), p(rgb)), b"NULL"),
           (lambda: L.crt_shoot_rays(tracer.ctx, p(rays), 64, 2, C.byref(opt), None), b"NULL"),
           (lambda: L.crt_shoot_rays(tracer.ctx, p(rays), 64, 2, None, p(rgb)), b"NULL"),
           (lambda: L.crt_shoot_rays(tracer.ctx, p(rays), 64, 4, C.byref(opt), p(rgb)), b"ray_type"),
           (lambda: L.crt_shoot_rays(tracer.ctx, p(rays), 64, 2, C.byref(gi), p(rgb)), b"use_gi"),
           (lambda: L.crt_shoot_rays(tracer.ctx, p(rays), 64, 2, C.byref(deep), p(rgb)), b"max_depth"),
           (lambda: L.crt_shoot_rays_device(tracer.ctx, None, 64, 2, C.byref(opt), None, None), b"NULL"),
           (lambda: L.crt_shoot_rays_device(tracer.ctx, p(rays), 64, 2, None, p(rgb), None), b"NULL"),
           (lambda: L.crt_shoot_rays_device(tracer.ctx, p(rays), 64, 9, C.byref(opt), p(rgb), None), b"ray_type"),
           (lambda: L.crt_shoot_rays_device(tracer.ctx, p(rays), 64, 2, C.byref(gi), p(rgb), None), b"use_gi"),
           (lambda: L.crt_shoot_rays_device(tracer.ctx, p(rays), 64, 2, C.byref(deep), p(rgb), None), b"max_depth")]
    for k, (call, word) in enumerate(bad):
        assert call() == pkg.CRT_ERR_INVALID, k
        assert word in L.crt_last_error(tracer.ctx), (k, L.crt_last_error(tracer.ctx))
    assert np.all(rgb == 5.0), "a refused call writes nothing"
    assert L.crt_shoot_rays(tracer.ctx, None, 0, 9, None, None) == pkg.CRT_OK, "n == 0 touches nothing, whatever else is passed"
    assert tracer.shoot_rays(np.zeros((0, 6), dtype=np.float32)).shape == (0, 3)
    with pytest.raises(ValueError):
        tracer.shoot_rays(np.zeros((4, 5), dtype=np.float32))
    # max_depth 63 is the deepest a frame takes, and a radiance query with it
    assert_same_floats(tracer.shoot_rays(rays, max_depth=63), sh.oracle_colours(c["oracle"], rays, 63), "max_depth 63")
    assert_same_floats(tracer.shoot_rays(c["rays"], max_depth=c["depth"]), c["want"], "query after the errors")


def test_multi_device_tracer_refuses_radiance_queries(pkg, scenes):
    scene, _, _ = small_case(scenes, "hw07")
    tracer = pkg.Tracer(pkg.Scene(json_text=scenes.to_json(scene)), devices=[0, 0])
    with pytest.raises(RuntimeError, match="multi-device"):
        tracer.shoot_rays(np.zeros((8, 6), dtype=np.float32))
    with pytest.raises(RuntimeError, match="multi-device"):
        tracer.shoot_rays_device(0, 8, 0)
    with pytest.raises(RuntimeError, match="multi-device"):
        tracer.shoot_stats()
