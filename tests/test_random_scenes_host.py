"""The seeded random scenes of tests/random_scene_sets.py on the CPU: the conditions their seeds have to meet (every route of the ray
tree occurs; the candidate filter keeps at least three quarters of the scenes), the oracle against the live reference on every seed
(skipped where oracle/_ref is absent), and the fixture tests/golden/random_scenes.npz."""
import os

import numpy as np
import pytest

import random_scene_sets as rss
from helpers import assert_same_hits

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "random_scenes.npz")


def test_the_generator_is_a_pure_function_of_its_arguments(scenes):
    for seed in rss.SEEDS[:4]:
        a, b = rss.seed_scene(seed), rss.seed_scene(seed)
        assert scenes.to_blob(a) == scenes.to_blob(b) and scenes.to_json(a) == scenes.to_json(b)
        assert 1 <= len(a["objects"]) <= 12 and 0 <= len(a["lights"]) <= 4 and 1 <= rss.depth_of(a) <= 5
        narrowed = rss.make(seed, 48, 32, keep_meshes=[0], keep_lights=[])
        assert len(narrowed["objects"]) == 1 and narrowed["lights"] == []
        assert np.array_equal(narrowed["objects"][0]["vertices"], rss.make(seed, 48, 32)["objects"][0]["vertices"])
    assert len(rss.SEEDS) == 24 == len(set(rss.SEEDS)) and sum(rss.frame_size(s) == (50, 30) for s in rss.SEEDS) == 6
    assert set(rss.FIXTURE_SEEDS) <= set(rss.SEEDS) and set(rss.GI_SEEDS) <= set(rss.SEEDS) and len(rss.FIXTURE_SEEDS) == len(rss.GI_SEEDS) == 8


def test_every_route_occurs_over_the_seeds(scenes, oracle):
    """check_census: a condition on the inputs.  The census walks the ray trees in numpy around the oracle's trace and occlusion calls;
    that it walks the ORACLE's trees shows in the counters: rays, shaded hits, light evaluations and texel fetches equal render's."""
    total = {}
    for seed in rss.SEEDS:
        scene = rss.seed_scene(seed)
        o = oracle.OracleScene(scenes.to_blob(scene))
        _, counters = o.render(rss.depth_of(scene))
        c = rss.census(scene, o)
        assert c["counters"] == {k: counters[k] for k in c["counters"]}, seed
        vn = [o.mesh_normals(m)[1][np.unique(ob["triangles"])] for m, ob in enumerate(scene["objects"])]
        assert all(np.isfinite(n).all() and (np.abs(n).sum(axis=1) > 0).all() for n in vn), "seed %d: a zero vertex normal" % seed
        rss.add_census(total, c)
    print("census over %d seeds: %r" % (len(rss.SEEDS), total))
    rss.check_census(total)


def test_the_filter_keeps_three_quarters_of_the_scenes(pkg, scenes, tmp_path):
    kept = [seed for seed in rss.SEEDS if rss.filter_accepts(pkg, scenes, rss.seed_scene(seed), str(tmp_path))]
    print("filter keeps %d of %d: %r" % (len(kept), len(rss.SEEDS), kept))
    assert 4 * len(kept) >= 3 * len(rss.SEEDS)


def compare(got, want, what, types, depths):
    for t in types:
        assert_same_hits(got["hits"][t], want["hits"][t], "%s: hits of type %d" % (what, t))
    for rule in ("occ", "occ_gi"):
        bad = np.flatnonzero(np.asarray(got[rule], dtype=bool) != np.asarray(want[rule], dtype=bool))
        assert bad.size == 0, "%s %s: %d of %d rays differ, first %d" % (what, rule, bad.size, len(got[rule]), bad[0])
    for t in rss.RAY_TYPES:
        for d in depths:
            rss.assert_same_frame(got["shoot"][(t, d)], want["shoot"][(t, d)], "%s: shootRay type %d depth %d" % (what, t, d))


@pytest.mark.parametrize("seed", rss.SEEDS)
def test_oracle_equals_the_live_reference(oracle, scenes, seed):
    import reference_ray_sets as rrs
    if not (oracle.reference_available(True) and oracle.reference_available(False)):
        pytest.skip("oracle/_ref not built here")
    scene = rss.seed_scene(seed)
    depth, blob = rss.depth_of(scene), scenes.to_blob(scene)
    o = oracle.OracleScene(blob)
    want_frame, _ = oracle.reference_render(blob, max_depth=depth)
    rss.assert_same_frame(o.render(depth)[0], want_frame, "seed %d: frame at depth %d" % (seed, depth))
    rays, depths = rss.rays(scene, seed, 256, o), sorted({1, depth})
    dist = rss.distances(seed, len(rays))
    hits = oracle.reference_trace(blob, rays, rss.RAY_TYPES, textured=True)
    shoot = oracle.reference_shoot(blob, rays, rss.RAY_TYPES, depths)
    want = {"hits": {t: rrs.crt_hits(scene, hits[k]) for k, t in enumerate(rss.RAY_TYPES)}, "occ": oracle.reference_occluded(blob, rays, dist),
            "occ_gi": oracle.reference_occluded(blob, rays, dist, gi=True),
            "shoot": {(t, d): np.ascontiguousarray(shoot[i, j]) for i, t in enumerate(rss.RAY_TYPES) for j, d in enumerate(depths)}}
    assert int(want["hits"][2]["hit"].sum()) >= 20, "seed %d: the rays must meet the scene" % seed
    compare(rss.oracle_answers(o, scene, rays, dist, depths), want, "seed %d" % seed, rss.RAY_TYPES, depths)


@pytest.mark.parametrize("seed", rss.FIXTURE_SEEDS)
def test_oracle_equals_the_fixture(oracle, scenes, seed):
    """the recorded answers of the real reference (tests/golden/random_scenes.npz), wherever the oracle builds"""
    fx = rss.load_fixture()[seed]
    scene = rss.make(seed, *rss.FIXTURE_SIZE)
    depth = int(np.ravel(fx["depth"])[0])
    assert depth == rss.depth_of(scene)
    o = oracle.OracleScene(scenes.to_blob(scene))
    rss.assert_same_frame(o.render(depth)[0], fx["frame"], "seed %d: frame" % seed)
    assert np.array_equal(rss.rays(scene, seed, rss.FIXTURE_RAYS, o).view(np.uint32), fx["rays"].view(np.uint32)), "the seed's rays are the fixture's"
    want = {"hits": {t: fx["hits_%d" % t] for t in rss.HIT_TYPES}, "occ": fx["occ"], "occ_gi": fx["occ_gi"],
            "shoot": {(t, depth): fx["shoot"][k] for k, t in enumerate(rss.RAY_TYPES)}}
    compare(rss.oracle_answers(o, scene, fx["rays"], fx["dist"], [depth], rss.HIT_TYPES), want, "seed %d" % seed, rss.HIT_TYPES, [depth])


def test_the_fixture_is_what_its_script_writes(oracle):
    if not (oracle.reference_available(True) and oracle.reference_available(False)):
        pytest.skip("oracle/_ref not built here")
    from golden import make_random_scenes
    with open(GOLDEN, "rb") as f:
        committed = f.read()
    assert len(committed) <= 190 * 1024
    assert make_random_scenes.fixture_bytes() == committed
