"""Radiance queries in the GI mode on the GPU (include/crt_hip.h: crt_shoot_rays_gi*).  The oracle has GI frames, not GI rays: with one
ray per pixel, pixel p of a GI frame is (0 + shootRay(centre ray, key p)) * (1 / 1) with key p = mix(mix(seed, p), 0) -- the query's
colour for the camera's rays shot as PRIMARY rays with those keys.  Colours are compared as float values, NaNs equal (`0 + c` turns a
-0 into +0 and changes nothing else); two answers of the query itself are compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import query_sets as qs
import shoot_gi_sets as gs
import shoot_sets as sh
from helpers import level_rays, same_bits
from shoot_gi_sets import case, gi_options

pytestmark = pytest.mark.gpu
N = gs.W * gs.H


def shoot_device(tracer, rays, keys, options, ray_type=qs.RAY_PRIMARY):
    import torch
    n = len(rays)
    d_rays = torch.from_numpy(np.array(rays)).cuda()
    d_keys = torch.from_numpy(np.array(keys).view(np.int32)).cuda() if keys is not None else None
    d_rgb = torch.full((n + 1, 3), float("nan"), dtype=torch.float32, device="cuda")   # (one row more: must stay untouched)
    torch.cuda.synchronize()
    tracer.shoot_rays_gi_device(d_rays.data_ptr(), n, d_rgb.data_ptr(), d_keys.data_ptr() if d_keys is not None else None, ray_type, options)
    torch.cuda.synchronize()
    rgb = d_rgb.cpu().numpy()
    assert np.all(np.isnan(rgb[n:])), "written past the end"
    return rgb[:n]


def stats_tuple(st):
    return (st.rays, st.levels, level_rays(st), st.shadow_records, st.rerouted)


def check_frame_case(pkg, scenes, oracle, c, name, depth, samples, camera=None):
    tracer, rays, keys = c["tracer"], c["rays"], c["keys"]
    opt = gi_options(pkg, depth, samples)
    want = gs.gi_frame(scenes, oracle, name, depth, samples, camera=camera).reshape(N, 3)
    own = tracer.render(options=opt).reshape(N, 3).copy()
    dev = shoot_device(tracer, rays, None, opt)
    st = tracer.shoot_stats()
    print("%s %s d%d S%d: levels %d level_rays %s shadow_records %d rerouted %d kernel %.3f ms" % (
        name, camera or "", depth, samples, st.levels, level_rays(st)[:st.levels], st.shadow_records, st.rerouted, st.kernel_ms))
    what = "%s %s depth %d samples %d" % (name, camera or "", depth, samples)
    gs.assert_same_values(dev, want, what + ": the oracle's GI frame")
    gs.assert_same_values(dev, own, what + ": this library's GI frame")
    same_bits(shoot_device(tracer, rays, keys, opt), dev, what + ": explicit keys, device")
    same_bits(tracer.shoot_rays_gi(rays, keys, qs.RAY_PRIMARY, opt), dev, what + ": explicit keys, host variant")
    same_bits(tracer.shoot_rays_gi(rays, None, qs.RAY_PRIMARY, max_depth=depth, gi_sample_size=samples, gi_seed=gs.SEED), dev, what + ": keys=NULL, host variant")
    assert st.rays == N == level_rays(st)[0] and 1 <= st.levels <= depth + 1
    fan = max(2, samples)
    assert all(level_rays(st)[g + 1] <= fan * level_rays(st)[g] for g in range(63))


# ---- 1. the GI frame is a special case
@pytest.mark.parametrize("depth,samples", gs.TUPLES)
@pytest.mark.parametrize("name", list(gs.SCENES))
def test_the_gi_frame_is_a_special_case(pkg, scenes, oracle, name, depth, samples, tmp_path_factory):
    check_frame_case(pkg, scenes, oracle, case(pkg, scenes, oracle, name, tmp_path_factory), name, depth, samples)


@pytest.mark.parametrize("camera", list(gs.CAMERAS))
def test_the_gi_frame_from_other_cameras(pkg, scenes, oracle, camera, tmp_path_factory):
    check_frame_case(pkg, scenes, oracle, case(pkg, scenes, oracle, "hw11", tmp_path_factory, camera=camera), "hw11", 3, 2, camera=camera)


# ---- 2. the statistics are not vacuous
def test_stats_are_not_vacuous(pkg, scenes, oracle, tmp_path_factory):
    c = case(pkg, scenes, oracle, "hw11", tmp_path_factory)
    c["tracer"].shoot_rays_gi(c["rays"], None, qs.RAY_PRIMARY, gi_options(pkg, 3, 2))
    st = c["tracer"].shoot_stats()
    lr = level_rays(st)
    print("hw11 (3, 2): levels %d level_rays %s shadow_records %d" % (st.levels, lr[:st.levels], st.shadow_records))
    assert st.levels == 4
    assert lr[1] > lr[0], "diffuse hits dominate and each spawns two"
    assert st.shadow_records > lr[0]
    assert c["tracer"].query_stats().rays == N


# ---- 3. a colour belongs to (ray, key), not to the batch
def test_a_colour_belongs_to_its_ray_and_key(pkg, scenes, oracle, tmp_path_factory):
    c = case(pkg, scenes, oracle, "hw14", tmp_path_factory)
    tracer, rays, keys = c["tracer"], c["rays"], c["keys"]
    opt = gi_options(pkg, 3, 2)
    full = tracer.shoot_rays_gi(rays, keys, qs.RAY_PRIMARY, opt)
    full_stats = stats_tuple(tracer.shoot_stats())
    gs.assert_same_values(full, gs.gi_frame(scenes, oracle, "hw14", 3, 2).reshape(N, 3), "hw14: the full set")
    same_bits(tracer.shoot_rays_gi(rays, keys, qs.RAY_PRIMARY, opt), full, "two identical calls")
    perm = np.random.default_rng(5).permutation(N)
    same_bits(tracer.shoot_rays_gi(rays[perm], keys[perm], qs.RAY_PRIMARY, opt), full[perm], "a permutation of the (ray, key) pairs")
    same_bits(shoot_device(tracer, rays[perm], keys[perm], opt), full[perm], "a permutation, device variant")
    for n in (1, 63, 64, 65, 257):
        got = tracer.shoot_rays_gi(rays[:n], keys[:n], qs.RAY_PRIMARY, opt)
        st = tracer.shoot_stats()
        assert got.shape == (n, 3) and st.rays == n == level_rays(st)[0]
        same_bits(got, full[:n], "the first %d pairs" % n)
    # other keys, other colours: the keys are read
    other = tracer.shoot_rays_gi(rays, keys[::-1], qs.RAY_PRIMARY, opt)
    assert gs.differing_pixels(other, full) > N // 2
    # the chunk loops: 64 rays per pass and host round trip, 128 per launch
    tracer.set_query_chunks(64, 128, 64)
    try:
        same_bits(tracer.shoot_rays_gi(rays, keys, qs.RAY_PRIMARY, opt), full, "in passes of 64, host variant")
        assert stats_tuple(tracer.shoot_stats()) == full_stats
        same_bits(shoot_device(tracer, rays, keys, opt), full, "in passes of 64, device variant")
        assert stats_tuple(tracer.shoot_stats()) == full_stats
        same_bits(shoot_device(tracer, rays, None, opt), full, "in passes of 64, keys=NULL: a pass's keys start at its first ray's index")
        same_bits(tracer.shoot_rays_gi(rays, None, qs.RAY_PRIMARY, opt), full, "in passes of 64, keys=NULL, host variant")
    finally:
        tracer.set_query_chunks(0, 0, 0)


# ---- 4. arbitrary rays, zero samples, no refractive mesh
def test_arbitrary_rays_without_samples_are_the_plain_query(pkg, scenes, oracle, tmp_path_factory):
    c = case(pkg, scenes, oracle, "hw08", tmp_path_factory)
    tracer = c["tracer"]
    # any origin and direction; (random_rays' directions are unit vectors:) 256 of them scaled, four zero directions, a NaN origin
    rays = qs.random_rays()
    rays[:256, 3:] *= np.float32(3.0)
    rays[256:260, 3:] = 0.0
    rays[260, 0] = np.nan
    assert rays.shape == (4096, 6)
    plain = tracer.shoot_rays(rays, qs.RAY_REFLECTION, max_depth=3)
    plain_stats = tracer.shoot_stats()
    got = tracer.shoot_rays_gi(rays, None, qs.RAY_REFLECTION, gi_options(pkg, 3, 0))
    st = tracer.shoot_stats()
    print("hw08 random rays: levels %d level_rays %s shadow_records %d rerouted %d" % (st.levels, level_rays(st)[:st.levels], st.shadow_records, st.rerouted))
    gs.assert_same_values(got, plain, "hw08, no samples: crt_shoot_rays' colours")
    assert st.rerouted > 0 and stats_tuple(st) == stats_tuple(plain_stats)
    same_bits(shoot_device(tracer, rays, None, gi_options(pkg, 3, 0), qs.RAY_REFLECTION), got, "device variant")


# ---- 5. the occlusion rule by its own door
def test_the_occlusion_rule_alone(pkg, scenes, oracle, tmp_path_factory):
    c = case(pkg, scenes, oracle, "hw11", tmp_path_factory)
    tracer, rays = c["tracer"], c["rays"]
    got = tracer.shoot_rays_gi(rays, None, qs.RAY_PRIMARY, gi_options(pkg, 3, 0))
    gs.assert_same_values(got, gs.gi_frame(scenes, oracle, "hw11", 3, 0).reshape(N, 3), "hw11, no samples: the oracle's GI frame")
    plain = tracer.shoot_rays(rays, qs.RAY_PRIMARY, max_depth=3)
    differing = gs.differing_pixels(got, plain)
    print("hw11, no samples: %d of %d pixels differ from crt_shoot_rays (the oracle: 285; 249 without the last two rows)" % (differing, N))
    assert differing >= 100


# ---- 6. every walk route
def test_every_walk_route(pkg, scenes, oracle, tmp_path_factory):
    opt = gi_options(pkg, 3, 2)
    want = gs.gi_frame(scenes, oracle, "hw11", 3, 2).reshape(N, 3)
    colours = {}
    for tag, tuning in (("default", None), ("bvh=0", dict(bvh=0)), ("bvh=2", dict(bvh=2))):
        c = case(pkg, scenes, oracle, "hw11", tmp_path_factory, tuning=tuning)
        colours[tag] = shoot_device(c["tracer"], c["rays"], c["keys"], opt)
        st = c["tracer"].shoot_stats()
        print("%s: levels %d level_rays %s shadow_records %d rerouted %d" % (tag, st.levels, level_rays(st)[:st.levels], st.shadow_records, st.rerouted))
        gs.assert_same_values(colours[tag], want, "hw11 " + tag)
        if tag == "bvh=0":
            assert st.rerouted >= st.shadow_records > 0 and st.rerouted >= st.rays, "the reference-order walk for everything"
    same_bits(colours["bvh=0"], colours["default"], "bvh=0 against the default")
    same_bits(colours["bvh=2"], colours["default"], "bvh=2 against the default")


# ---- 7. arguments
def test_bad_arguments_are_errors_and_nothing_else_changes(pkg, scenes, oracle, tmp_path_factory):
    c = case(pkg, scenes, oracle, "hw11", tmp_path_factory)
    tracer, L = c["tracer"], pkg.lib()
    rays = np.ascontiguousarray(qs.random_rays()[:64])
    keys = np.arange(64, dtype=np.uint32)
    rgb = np.full((64, 3), 5.0, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    frame_before = tracer.render(max_depth=3).copy()
    s0 = tracer.stats()
    opt = gi_options(pkg, 3, 2)
    plain, wide, deep = pkg.make_options(3), gi_options(pkg, 3, 65), gi_options(pkg, 64, 2)
    bad = [(lambda: L.crt_shoot_rays_gi(tracer.ctx, p(rays), p(keys), 64, 2, C.byref(plain), p(rgb)), b"crt_shoot_rays'"),
           (lambda: L.crt_shoot_rays_gi(tracer.ctx, p(rays), p(keys), 64, 2, C.byref(plain), p(rgb)), b"use_gi"),
           (lambda: L.crt_shoot_rays_gi(tracer.ctx, p(rays), p(keys), 64, 2, C.byref(wide), p(rgb)), b"gi_sample_size"),
           (lambda: L.crt_shoot_rays_gi(tracer.ctx, p(rays), p(keys), 64, 2, C.byref(deep), p(rgb)), b"max_depth"),
           (lambda: L.crt_shoot_rays_gi(tracer.ctx, p(rays), p(keys), 64, 4, C.byref(opt), p(rgb)), b"ray_type"),
           (lambda: L.crt_shoot_rays_gi(tracer.ctx, None, p(keys), 64, 2, C.byref(opt), p(rgb)), b"NULL"),
           (lambda: L.crt_shoot_rays_gi(tracer.ctx, p(rays), p(keys), 64, 2, None, p(rgb)), b"NULL"),
           (lambda: L.crt_shoot_rays_gi(tracer.ctx, p(rays), p(keys), 64, 2, C.byref(opt), None), b"NULL"),
           (lambda: L.crt_shoot_rays_gi_device(tracer.ctx, p(rays), None, 64, 2, C.byref(plain), p(rgb), None), b"use_gi"),
           (lambda: L.crt_shoot_rays_gi_device(tracer.ctx, p(rays), None, 64, 2, C.byref(wide), p(rgb), None), b"gi_sample_size"),
           (lambda: L.crt_shoot_rays_gi_device(tracer.ctx, p(rays), None, 64, 2, C.byref(deep), p(rgb), None), b"max_depth"),
           (lambda: L.crt_shoot_rays_gi_device(tracer.ctx, p(rays), None, 64, 9, C.byref(opt), p(rgb), None), b"ray_type"),
           (lambda: L.crt_shoot_rays_gi_device(tracer.ctx, None, None, 64, 2, C.byref(opt), p(rgb), None), b"NULL"),
           (lambda: L.crt_shoot_rays_gi_device(tracer.ctx, p(rays), None, 64, 2, None, p(rgb), None), b"NULL"),
           (lambda: L.crt_shoot_rays_gi_device(tracer.ctx, p(rays), None, 64, 2, C.byref(opt), None, None), b"NULL")]
    for k, (call, word) in enumerate(bad):
        assert call() == pkg.CRT_ERR_INVALID, k
        assert word in L.crt_last_error(tracer.ctx), (k, L.crt_last_error(tracer.ctx))
    assert np.all(rgb == 5.0), "a refused call writes nothing"
    assert L.crt_shoot_rays_gi(tracer.ctx, None, None, 0, 9, None, None) == pkg.CRT_OK, "n == 0 touches nothing, whatever else is passed"
    assert L.crt_shoot_rays_gi_device(tracer.ctx, None, None, 0, 9, None, None, None) == pkg.CRT_OK
    assert tracer.shoot_rays_gi(np.zeros((0, 6), dtype=np.float32), max_depth=3).shape == (0, 3)
    with pytest.raises(ValueError):
        tracer.shoot_rays_gi(rays, keys[:63], max_depth=3)
    with pytest.raises(TypeError):
        tracer.shoot_rays_gi(rays, keys, options=opt, max_depth=3)

    # the pass-size rule, on a context that has run nothing
    fresh = pkg.Tracer(pkg.Scene(json_text=scenes.to_json(c["scene"])))
    huge = gi_options(pkg, 40, 64)
    assert L.crt_shoot_rays_gi(fresh.ctx, p(rays), p(keys), 64, 2, C.byref(huge), p(rgb)) == pkg.CRT_ERR_INVALID
    message = L.crt_last_error(fresh.ctx)
    assert b"max(2, gi_sample_size)^max_depth" in message and b"64^40" in message, message
    assert np.all(rgb == 5.0) and fresh.shoot_stats().rays == 0 and fresh.query_stats().rays == 0, "no kernel has run"
    # the deepest a pass of 64 rays can be: 64 x 2^20 = 2^26
    assert L.crt_shoot_rays_gi(fresh.ctx, p(rays), p(keys), 64, 2, C.byref(gi_options(pkg, 21, 2)), p(rgb)) == pkg.CRT_ERR_INVALID
    assert b"2^21" in L.crt_last_error(fresh.ctx), L.crt_last_error(fresh.ctx)

    # after a GI call
    got = tracer.shoot_rays_gi(rays, keys, qs.RAY_REFLECTION, opt)
    assert got.shape == (64, 3) and tracer.shoot_stats().rays == 64
    assert L.crt_shoot_rays(tracer.ctx, p(rays), 64, 2, C.byref(opt), p(rgb)) == pkg.CRT_ERR_INVALID and b"use_gi" in L.crt_last_error(tracer.ctx)
    assert np.all(rgb == 5.0)
    from helpers import assert_same_floats
    assert_same_floats(tracer.shoot_rays(rays, qs.RAY_REFLECTION, max_depth=3), sh.oracle_colours(c["oracle"], rays, 3), "a plain query after a GI query")
    assert_same_floats(tracer.render(max_depth=3), frame_before, "a frame after a GI query")
    s1 = tracer.stats()
    assert (s1.fallback_frames, s1.queue_bytes) == (s0.fallback_frames, s0.queue_bytes)


def test_multi_device_tracer_refuses_gi_radiance_queries(pkg, scenes):
    tracer = pkg.Tracer(pkg.Scene(json_text=scenes.to_json(gs.scene_of(scenes, "hw08"))), devices=[0, 0])
    with pytest.raises(RuntimeError, match="multi-device"):
        tracer.shoot_rays_gi(np.zeros((8, 6), dtype=np.float32))
    with pytest.raises(RuntimeError, match="multi-device"):
        tracer.shoot_rays_gi_device(0, 8, 0)
