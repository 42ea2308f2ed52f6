"""Texture lookup on the GPU (csrc/kernel_common.h: texture_color) against the REAL reference's recorded answers for the texture cards of
tests/texture_sets.py (tests/golden/texture_rays.npz): non-square bitmaps with distinct texels, UVs beyond the unit square and at
every class of the reference's x86 float-to-integer conversions, checker squares of 0, infinity, 1e-20 and a negative size, edge widths
of 0, 1/3, 0.5 and below zero.  Frames on every kernel path, the ray, lighting and radiance queries, the multi-part tracer: bit for bit
(two NaNs are equal).  The GI builds instantiate the same function: their frame and radiance query against the oracle, which
tests/test_texture_host.py holds to the same fixture."""
import numpy as np
import pytest

import shade_sets as ss
import texture_sets as ts
from helpers import assert_same_floats, assert_same_hits, assert_shaded
from test_gpu_random_scenes import TUNINGS, tuning_id

pytestmark = pytest.mark.gpu
_CASES = {}


def case(pkg, scenes, name, tmp_path_factory):
    """the fixture's scene through the .crtscene and P6 route, and a tracer with the default tuning: made once"""
    if name not in _CASES:
        fx = ts.load_fixture()[name]
        scene = ts.make(name)
        assert ts.blob(scene) == fx["blob"], name + ": the generator's scene is not the fixture's"
        folder = str(tmp_path_factory.mktemp("cards_" + name))
        scenes.write_bitmaps(scene, folder)
        host = pkg.Scene(json_text=ts.to_json(scene), folder=folder)
        _CASES[name] = dict(scene=scene, fx=fx, host=host, tracer=pkg.Tracer(host), rays=np.ascontiguousarray(fx["rays"]))
    return _CASES[name]


# ---- 1. frames
@pytest.mark.parametrize("tuning", TUNINGS, ids=tuning_id)
@pytest.mark.parametrize("name", ts.GPU_SCENES)
def test_frame_equals_the_reference_on_every_kernel_path(pkg, scenes, name, tuning, tmp_path_factory):
    c = case(pkg, scenes, name, tmp_path_factory)
    tracer = pkg.Tracer(c["host"], tuning=pkg.make_tuning(**tuning)) if tuning else c["tracer"]
    for frame in ("first", "second"):       # the second frame of a context sizes (or leaves out) launches by the first frame's counters
        what = "%s, tuning %s, %s frame" % (name, tuning_id(tuning), frame)
        assert_same_floats(tracer.render(max_depth=ts.FRAME_DEPTH), c["fx"]["frame"], what)
        assert tracer.stats().fallback_frames == 0, what


@pytest.mark.parametrize("name", ts.GPU_SCENES)
def test_counting_build_equals_the_reference(pkg, scenes, name, tmp_path_factory):
    c = case(pkg, scenes, name, tmp_path_factory)
    assert_same_floats(c["tracer"].render(max_depth=ts.FRAME_DEPTH, counters=True), c["fx"]["frame"], name + ", counting build")
    assert c["tracer"].stats().counters_valid == 1


def test_two_parts_equal_the_reference(pkg, scenes, tmp_path_factory):
    c = case(pkg, scenes, "shapes", tmp_path_factory)
    tracer = pkg.Tracer(c["host"], devices=[0, 0])
    assert_same_floats(tracer.render(max_depth=ts.FRAME_DEPTH), c["fx"]["frame"], "shapes, two parts")


# ---- 2. queries
@pytest.mark.parametrize("name", ts.GPU_SCENES)
def test_hit_records_lighting_and_radiance_equal_the_reference(pkg, scenes, name, tmp_path_factory):
    """trace_rays gives the reference's records, u and v included; shade_hits on THOSE records and shoot_rays on the rays give the
    reference's colours (every direction is a fixed point of shootRay's normalisation, tests/shade_sets.py)."""
    c = case(pkg, scenes, name, tmp_path_factory)
    tracer, fx, rays = c["tracer"], c["fx"], c["rays"]
    assert ss.is_fixed_point(rays).all()
    want = fx["hits"].astype(pkg.HIT_DTYPE)
    got = tracer.trace_rays(rays, ts.RAY_TYPE)
    assert_same_hits(got, want, name + ": trace_rays")
    rgb, status = tracer.shade_hits(got)
    assert_shaded(pkg, rgb, status, ss.expected_status(pkg, c["scene"], want), fx["shoot"][ts.DEPTHS[0]], name + ": shade_hits")
    assert int((status == pkg.SHADE_DIFFUSE).sum()) >= 0.8 * len(rays)
    for d in ts.DEPTHS:
        assert_same_floats(tracer.shoot_rays(rays, ts.RAY_TYPE, max_depth=d), fx["shoot"][d], "%s: shoot_rays at depth %d" % (name, d))


# ---- 3. the GI builds
@pytest.mark.parametrize("name", ts.GPU_SCENES)
def test_gi_frame_and_gi_radiance_query_equal_the_oracle(pkg, scenes, oracle, name, tmp_path_factory):
    c = case(pkg, scenes, name, tmp_path_factory)
    tracer, rays, depth = c["tracer"], c["rays"], 2
    o = oracle.OracleScene(c["fx"]["blob"])
    fields = dict(use_gi=1, gi_sample_size=1, rays_per_pixel=2, gi_seed=77)
    options = pkg.make_options(depth, **dict(fields, use_gi=True))
    want, _ = o.render(options=oracle.make_options(depth, **fields))
    assert_same_floats(tracer.render(options=options), want, name + ": GI frame")
    keys = np.random.default_rng(5).integers(0, 1 << 32, len(rays), dtype=np.uint64).astype(np.uint32)
    want = o.shoot_gi(rays, keys, ts.RAY_TYPE, oracle.make_options(depth, **fields))
    assert_same_floats(tracer.shoot_rays_gi(rays, keys, ts.RAY_TYPE, options), want, name + ": shoot_rays_gi")
