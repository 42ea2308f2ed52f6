"""The oracle against the real reference binary, on scenes that are NOT in tests/golden/.  Runs where
oracle/_ref/ exists (built from /root/reference in the development container; shipped to the GPU box as a
binary); skipped elsewhere."""
import numpy as np
import pytest

import degenerate_sets
import reference_ray_sets as rrs
import scale_sets
from helpers import assert_same_floats, assert_same_hits


def _have(oracle, textured):
    return oracle.reference_available(textured=textured)


@pytest.mark.parametrize("name,w,h,detail,depth", [
    ("hw08", 96, 64, 0.3, 1),
    ("hw11", 128, 72, 0.2, 5),
    ("hw14", 112, 63, 0.03, 8),
    ("hw12", 96, 54, 0.06, 3),
    # the benchmark scenes at FULL detail (the deep-tree paths: depth-25 cut-off, 8.6x leaf duplication, KDTree.cpp:10-46)
    ("hw14", 160, 90, 1.0, 8),     # 207,954 triangles
    ("hw12", 160, 90, 1.0, 8),     # 60,156 triangles, 1024x1024 bitmap
    ("hw11", 160, 90, 1.0, 8),
])
def test_restatement_is_bit_exact(oracle, scenes, name, w, h, detail, depth):
    kw = {"bitmap_size": 32} if name == "hw12" and detail < 1.0 else {}
    scene = scenes.make(name, width=w, height=h, detail=detail, **kw)
    if not _have(oracle, bool(scene.get("textures"))):
        pytest.skip("oracle/_ref not built here")
    blob = scenes.to_blob(scene)
    want, _ = oracle.reference_render(blob, max_depth=depth)
    got, _ = oracle.OracleScene(blob).render(depth)
    assert_same_floats(got, want, name)


# the scenes of the scale tests (tests/scale_sets.py), at another frame size than their fixtures in tests/golden/
@pytest.mark.parametrize("base,case", [("hw11", "hi"), ("hw11", "lo"), ("hw11", "s1e3"), ("hw11", "offset"), ("hw11", "combined"), ("hw11", "s1e6"),
                                       ("hw14", "hi"), ("hw14", "lo")])
def test_restatement_is_bit_exact_at_scale(oracle, scenes, base, case):
    if not _have(oracle, False):
        pytest.skip("oracle/_ref not built here")
    blob = scenes.to_blob(scale_sets.make_case(scenes, base, case, width=80, height=45))
    want, _ = oracle.reference_render(blob, max_depth=3)
    got, _ = oracle.OracleScene(blob).render(3)
    assert len(np.unique(want.reshape(-1, 3), axis=0)) > 50          # a picture, not a blank frame
    assert_same_floats(got, want, "%s %s" % (base, case))


def test_restatement_is_bit_exact_on_ill_formed_triangles(oracle, scenes):
    # tests/degenerate_sets.py's `mixed` scene (zero-area, underflowing near-collinear and needle triangles) at another frame size than its fixture
    if not _have(oracle, True):
        pytest.skip("oracle/_ref not built here")
    scene, _ = degenerate_sets.build(scenes, "mixed")
    scene["settings"] = dict(scene["settings"], image_settings={"width": 72, "height": 48, "bucket_size": 16})
    blob = scenes.to_blob(scene)
    want, _ = oracle.reference_render(blob, max_depth=degenerate_sets.DEPTH)
    got, _ = oracle.OracleScene(blob).render(degenerate_sets.DEPTH)
    assert np.isnan(want).any()                                        # NaN winners are on this frame too
    assert_same_floats(got, want, "mixed")


def test_camera_change_matches_reference(oracle, scenes):
    if not _have(oracle, False):
        pytest.skip("oracle/_ref not built here")
    scene = scenes.make("hw11", width=96, height=54, detail=0.2)
    scene["camera"]["position"] = [0.35, 0.6, 0.2]
    c, s = np.float32(np.cos(0.2)), np.float32(np.sin(0.2))
    scene["camera"]["matrix"] = [c, 0, -s, 0, 1, 0, s, 0, c]
    blob = scenes.to_blob(scene)
    want, _ = oracle.reference_render(blob, max_depth=4)
    o = oracle.OracleScene(scenes.to_blob(scenes.make("hw11", width=96, height=54, detail=0.2)))
    o.set_camera(scene["camera"]["position"], scene["camera"]["matrix"])  # same scene, camera set afterwards
    got, _ = o.render(4)
    assert_same_floats(got, want, "camera")


# the ray sets of the query fixtures (tests/reference_ray_sets.py) at ANOTHER seed: the oracle cannot be fitted to tests/golden/query_*.npz
@pytest.mark.parametrize("name", rrs.SCENES)
def test_single_rays_match_the_live_reference(oracle, scenes, name):
    if not (_have(oracle, True) and _have(oracle, False)):
        pytest.skip("oracle/_ref not built here")
    scene = rrs.make_scene(scenes, name)
    blob = scenes.to_blob(scene)
    o = oracle.OracleScene(blob)
    rs = rrs.build(scene, o, lambda rays, t: oracle.reference_trace(blob, rays, t, textured=True), rrs.LIVE_SEED)
    want = rrs.reference_answers(oracle, blob, scene, rs, name, check_plain=False)
    rrs.check_census(name, rrs.census(scene, rs, want))
    got = rrs.oracle_answers(o, scene, rs, lambda origin, direction, d: o.occluded(origin, direction, d, gi=True), name)
    assert np.array_equal(got["shoot_skip"], want["shoot_skip"])
    for cls in rrs.CLASSES:
        rows = np.flatnonzero(rs["labels"] == rrs.CLASSES.index(cls))
        for t in rrs.RAY_TYPES:
            assert_same_hits(got["hits"][t][rows], want["hits"][t][rows], "%s %s type %d" % (name, cls, t))
            for d in rrs.DEPTHS:
                assert_same_floats(got["shoot"][(t, d)][rows], want["shoot"][(t, d)][rows], "%s %s type %d depth %d" % (name, cls, t, d))
    for rule in ("occ", "occ_gi"):      # occ_gi: checkForIntersection with useGI, under which no mesh is skipped
        bad = np.flatnonzero(got[rule] != want[rule])
        assert bad.size == 0, "%s %s: %d of %d pairs differ, first: ray %d distance %r" % (name, rule, bad.size, len(got[rule]), rs["occ_index"][bad[0]],
                                                                                         rs["occ_dist"][bad[0]])


def test_shoot_ray_of_the_driver_is_the_frame_s_pixel(oracle, scenes):
    """oracle/ref_driver.cpp --rays sets renderOptions, useBounding and boundingType by hand instead of rendering a frame first: its
    shootRay of a camera ray has to be the colour render() gives that pixel (getRay's normalisation followed by shootRay's)."""
    if not _have(oracle, False):
        pytest.skip("oracle/_ref not built here")
    scene = scenes.make("hw11", width=64, height=36, detail=0.2)
    blob = scenes.to_blob(scene)
    frame, _ = oracle.reference_render(blob, max_depth=4)
    o = oracle.OracleScene(blob)
    rays = np.array([np.concatenate(o.camera_ray(r, c)) for r in range(o.height) for c in range(o.width)], dtype=np.float32)
    got = oracle.reference_shoot(blob, rays, 0, 4).reshape(frame.shape)
    rendered = (frame.view(np.uint32) != 0).any(axis=2)          # (the bucket grid may leave edge pixels unrendered: +0, 0, 0)
    assert rendered.sum() >= 0.9 * rendered.size and len(np.unique(frame.reshape(-1, 3), axis=0)) > 50
    assert_same_floats(got[rendered], frame[rendered], "shootRay of the camera rays against render()")


# the GI mode on matched (key, engine seed) pairs (tests/gi_reference_sets.py) that are NOT in tests/golden/gi_pairs_*.npz: the search
# repeated on another seed range and an eighth of the keys, the fixture's rays and pixels with the fresh pairs, the reference run now
LIVE_GI_SEEDS, LIVE_GI_KEYS = ((1 << 25) + 1, 1 << 23), (0, 1 << 29)


def test_gi_mode_matches_the_live_reference_on_fresh_pairs(oracle, scenes):
    import gi_reference_sets as grs
    if not _have(oracle, False):
        pytest.skip("oracle/_ref not built here")
    pairs = grs.find_pairs(oracle, *LIVE_GI_SEEDS, *LIVE_GI_KEYS)
    blob, fx = grs.load_fixture("hw11")
    print("fresh pairs: %d hit, %d jitter" % (len(pairs["hit"][0]), len(pairs["jitter"][0])))
    # expected 2^23 * 2^29 / 2^48 * 4/9 = 7 of each kind; the ranges are fixed, so the counts are too
    assert len(pairs["hit"][0]) >= 3 and len(pairs["jitter"][0]) >= 3
    assert not np.isin(pairs["hit"][1], fx["hit_seeds"]).any() and not np.isin(pairs["jitter"][1], fx["jitter_seeds"]).any()
    o = oracle.OracleScene(blob)
    live = grs.with_pairs(oracle, blob, fx, pairs, o.width)
    got = grs.oracle_answers(oracle, o, live)
    assert_same_floats(got["q_rgb"], live["q_rgb"], "shootRay, N = 1, MAX_DEPTH = 1")
    assert_same_floats(got["m_rgb"], live["m_rgb"], "shootRay below a mirror")
    assert_same_floats(got["p_rgb"], grs.frame_pixel(live["p_rgb"]), "frame pixels")
    assert np.array_equal(got["p_ray"].view(np.uint32), live["p_ray"].view(np.uint32)), "getRay(row, col, false)"
    assert np.array_equal(got["j_rays"].view(np.uint32), live["j_rays"].view(np.uint32)), "getRay(row, col, true)"
    assert (live["q_rgb"] != fx["q_rgb"]).any(axis=1).mean() > 0.8, "other draws, other colours"
