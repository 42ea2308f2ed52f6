"""The filter kernels' rarely taken routes (csrc/kernel_bvh.h, kernel_query.h, kernel_shade.h) on the GPU, bit for bit against the
oracle, each with proof that the route IS taken: the spilled part of the walk stack (the frame's high-water mark, SC_BVH_MARK, which
the tallying and the bounds-checked builds record: a walk is a function of its ray and kind alone, so the plain build's walks hold
as many entries), hits verified by bvh_leaf_walk, exact ties in distance, and give_up from a full stack (a test hook lowers the
stack).  The bounds-checked cases of a scene come first in this file: that build reads index 0 where the others would fault.

Deep stack: rare_sets.DEEP_N = 8192 cards.  The filter's build halves the cards (they lie evenly along a line) down to two per leaf
and folds two binary levels into one 4-wide node, and a walk along the line pushes every sibling it passes: three per 4-way node of
its path, one per 2-way node.  4096 cards: binary depth 11, depth:11/6 -- five 4-way levels and a 2-way one: 16 entries, measured 16 on
an MI355X, nothing spilled (2049 .. 4095 cards: the same or less).  8192 cards: depth:12/6, six 4-way levels on every path, the
stack's full 3 x 6 = 18 entries (19 allocated): measured 18 on an MI355X, under bvh=2 and under counters=2, for both cameras
(test_deep_stack_frames prints the marks)."""
import numpy as np
import pytest

import query_sets as qs
import rare_sets as rs
import shade_sets as ss
from helpers import assert_same_floats
from test_gpu_walk_fetch import MIXED_DEPTH, mixed_scene, tracer_of, violations

pytestmark = pytest.mark.gpu

BVH_LDS_STACK = 16       # csrc/kernel_common.h
SC_COUNT, SC_SHADOW = 0, 5 * 64     # csrc/kernel_common.h: rays per level; shadow rays queued
SC_BVH_MARK = 400 + 80   # csrc/kernel_bvh.h: the most entries any walk's stack held in the frame (tallying / bounds-checked builds)
DEEP_DEPTH = 3


def filter_note(tracer):
    note = tracer.kernels()["filter"]
    assert not note.startswith("none"), note
    return dict(kv.split(":") for kv in note.split(","))


def assert_same_records(got, want, what):
    for field in ("hit", "mesh", "triangle"):
        bad = np.flatnonzero(got[field] != want[field])
        assert bad.size == 0, "%s: %s differs for %d rays, first %d: got %r want %r" % (what, field, bad.size, bad[0], got[field][bad[0]], want[field][bad[0]])
    for field in ("t", "point", "normal", "u", "v"):
        assert_same_floats(got[field], want[field], "%s: %s" % (what, field))


# ------------------------------------------------------------------------------------------------------------------ deep stack
@pytest.fixture(scope="module")
def deep(pkg, scenes, oracle):
    scene = rs.deep_stack_scene()
    o = oracle.OracleScene(scenes.to_blob(scene))
    cam_a, cam_b = rs.deep_stack_cameras(rs.DEEP_N)
    frames = {}
    for name, cam in (("A", cam_a), ("B", cam_b)):
        o.set_camera(cam["position"], cam["matrix"])
        frames[name] = o.render(DEEP_DEPTH)[0].copy()
        frames[name].setflags(write=False)
    rays = rs.deep_stack_rays(o)          # (leaves camera A set)
    rays.setflags(write=False)
    return dict(scene=scene, oracle=o, cams={"A": cam_a, "B": cam_b}, frames=frames, rays=rays, cache={})


def deep_tracer(pkg, scenes, deep, **tuning):
    tracer = tracer_of(pkg, scenes, deep["scene"], **tuning)
    note = filter_note(tracer)
    wide = int(note["depth"].split("/")[1])
    assert 3 * wide + 1 > BVH_LDS_STACK, note
    return tracer


DEEP_TUNINGS = [("bvh=2", dict(bvh=2), False), ("counters=2", dict(), True), ("defaults", dict(), False), ("level_queue=0", dict(level_queue=0), False),
                ("level_queue=4097", dict(level_queue=1 | (1 << 12)), False), ("level_queue|512", "bit9", False)]


@pytest.mark.parametrize("name,tuning,tally", DEEP_TUNINGS, ids=[t[0] for t in DEEP_TUNINGS])
def test_deep_stack_frames(pkg, scenes, deep, name, tuning, tally):
    """Both cameras' frames at depth 3 are the oracle's on every launch path; the two builds that record it show walks holding more
    than the 16 entries that live in LDS (camera A: primary walks up the stack of cards, reflections and shadow walks back down it;
    camera B sees back faces only: its frame is the background and its mark is printed, not asserted), and the bounds-checked build -- spill index against its region's size, pushes against pops --
    records nothing."""
    if tuning == "bit9":
        tuning = dict(level_queue=int(pkg.make_tuning().level_queue) | 512)
    tracer = deep_tracer(pkg, scenes, deep, **tuning)
    assert tracer.kernels()["level0"].startswith("bvh_trace_")
    for cam in ("A", "B", "A"):
        tracer.set_camera(deep["cams"][cam]["position"], deep["cams"][cam]["matrix"])
        got = tracer.render(max_depth=DEEP_DEPTH, counters=2 if tally else False)
        counts = tracer.stream_counts()
        print("deep stack %s camera %s: filter %s, level-1 rays %d, shadow rays %d, stack high-water mark %d" % (
            name, cam, tracer.kernels()["filter"], counts[SC_COUNT + 1], counts[SC_SHADOW], counts[SC_BVH_MARK]))
        if tuning.get("bvh") == 2:
            assert violations(tracer) == []
        assert_same_floats(got, deep["frames"][cam], "deep stack, %s, camera %s" % (name, cam))
        assert tracer.stats().fallback_frames == 0
        if not (tally or tuning.get("bvh") == 2):
            assert counts[SC_BVH_MARK] == 0          # (the plain build records nothing)
        elif cam == "A":
            assert counts[SC_BVH_MARK] > BVH_LDS_STACK
        if cam == "A":
            assert counts[SC_COUNT + 1] > 0 and counts[SC_SHADOW] > 0


def deep_answers(pkg, deep, key):
    """The oracle's answers for the deep-stack ray set, computed once."""
    c, o, scene, rays = deep["cache"], deep["oracle"], deep["scene"], deep["rays"]
    if key not in c:
        if key in ("primary", "reflection"):
            c[key] = qs.oracle_hits(o, scene, rays, qs.RAY_PRIMARY if key == "primary" else qs.RAY_REFLECTION, pkg.HIT_DTYPE)
        elif key == "occluded":
            c[key] = qs.oracle_occluded(o, rays, deep_distances(rays))
        elif key == "shoot":
            c[key] = np.array([o.shoot(r[:3], r[3:], qs.RAY_REFLECTION, 0, DEEP_DEPTH) for r in rays], dtype=np.float32)
        c[key].setflags(write=False)
    return c[key]


def deep_distances(rays):
    """occlusion segments of every length: from a few cards to beyond the whole stack"""
    full = rs.DEEP_N * rs.DEEP_SPACING * np.sqrt(3.0)
    return (full * (0.02 + 1.1 * ((np.arange(len(rays)) * 0.6180339887) % 1.0))).astype(np.float32)


@pytest.fixture(scope="module")
def deep_query_tracer(pkg, scenes, deep):
    return deep_tracer(pkg, scenes, deep)


@pytest.mark.parametrize("kind", ["primary", "reflection"])
def test_deep_stack_trace_rays(pkg, deep, deep_query_tracer, kind):
    """Closest hits for both cameras' frame rays (whose walks the frames above show to spill) and the parallel bundle, both ways
    along the diagonal.  PRIMARY: the rays that run down the diagonal see back faces only and end in the miss check.  No ray of
    this scene leaves the filter: no in-plane ray, finite coordinates, unit directions, a stack of the built size."""
    want = deep_answers(pkg, deep, kind)
    cards = rs.first_hit_cards(deep["scene"], want)
    # first hits at every depth of the stack of cards (PRIMARY: the rays up the diagonal only, and each card stops a share of them)
    assert want["hit"].sum() > len(want) // 3 and (cards > rs.DEEP_N // 4).sum() > 50 and ((cards >= 0) & (cards < rs.DEEP_N // 8)).sum() > 50
    assert qs.non_finite_winners(want) == 0
    got = deep_query_tracer.trace_rays(deep["rays"], qs.RAY_PRIMARY if kind == "primary" else qs.RAY_REFLECTION)
    st = deep_query_tracer.query_stats()
    assert_same_records(got, want, "deep stack trace_rays %s" % kind)
    assert (st.rays, st.hits, st.rerouted) == (len(want), int(want["hit"].sum()), 0)


def test_deep_stack_occluded_rays(pkg, deep, deep_query_tracer):
    want = deep_answers(pkg, deep, "occluded")
    assert 0.2 < want.mean() < 0.98
    got = deep_query_tracer.occluded_rays(deep["rays"], deep_distances(deep["rays"]))
    st = deep_query_tracer.query_stats()
    assert np.array_equal(got, want), "occluded differs for %d rays" % int((got != want).sum())
    assert (st.rays, st.hits, st.rerouted) == (len(want), int(want.sum()), 0)


def test_deep_stack_shade_hits_and_light_points(pkg, scenes, oracle, deep, deep_query_tracer):
    """Direct lighting of the rays' hit records: the shadow rays of the light beside camera A run back through the stack of cards."""
    keep = ss.is_fixed_point(deep["rays"])
    rays, hits = deep["rays"][keep], deep_answers(pkg, deep, "reflection")[keep]
    assert len(rays) > 1000
    o = deep["oracle"]
    want = ss.oracle_colours(o, rays)
    status_want = ss.expected_status(pkg, deep["scene"], hits)
    diffuse = status_want == pkg.SHADE_DIFFUSE
    assert diffuse.sum() > 500 and len(np.unique(want[diffuse], axis=0)) > 100
    rgb, status = deep_query_tracer.shade_hits(hits)
    st = deep_query_tracer.query_stats()
    assert np.array_equal(status, status_want)
    exact = diffuse | (status_want == pkg.SHADE_BACKGROUND)
    assert_same_floats(rgb[exact], want[exact], "deep stack shade_hits")
    assert (st.rays, st.hits, st.rerouted) == (len(hits), int(diffuse.sum()), 0)
    white = oracle.OracleScene(scenes.to_blob(ss.white_scene(deep["scene"])))
    want_light = ss.oracle_colours(white, rays[diffuse])[:, 0]
    got_light = deep_query_tracer.light_points(hits["point"][diffuse].copy(), hits["normal"][diffuse].copy())
    st = deep_query_tracer.query_stats()
    assert_same_floats(got_light, want_light, "deep stack light_points")
    assert st.rerouted == 0 and np.any(got_light > 0)


def test_deep_stack_shoot_rays(pkg, deep, deep_query_tracer):
    want = deep_answers(pkg, deep, "shoot")
    assert len(np.unique(want, axis=0)) > 500
    got = deep_query_tracer.shoot_rays(deep["rays"], qs.RAY_REFLECTION, max_depth=DEEP_DEPTH)
    st = deep_query_tracer.shoot_stats()
    assert_same_floats(got, want, "deep stack shoot_rays at depth %d" % DEEP_DEPTH)
    assert st.rerouted == 0 and st.levels >= 2


# ---------------------------------------------------------------------------------------------------------- leaf walk and ties
@pytest.fixture(scope="module")
def leaf_walk(pkg, scenes, oracle):
    scene, large = rs.leaf_walk_scene()
    o = oracle.OracleScene(scenes.to_blob(scene))
    rays = rs.leaf_walk_rays()
    want = qs.oracle_hits(o, scene, rays, qs.RAY_REFLECTION, pkg.HIT_DTYPE)
    share_large, share_in_front = rs.leaf_walk_census(scene, large, rays, want)
    assert share_large >= 0.2 and share_in_front >= 0.2, (share_large, share_in_front)
    return dict(scene=scene, rays=rays, want=want, frame=o.render(2)[0])


@pytest.mark.parametrize("bvh", [2, 1])
def test_leaf_walk_winners(pkg, scenes, leaf_walk, bvh):
    """Winners verified by bvh_leaf_walk (the two large triangles, listed by every leaf of their mesh's tree) and small triangles in
    front of them, in a frame and as trace_rays records including mesh and triangle."""
    tracer = tracer_of(pkg, scenes, leaf_walk["scene"], bvh=bvh)
    assert int(filter_note(tracer)["walk_triangles"]) >= 2
    got = tracer.render(max_depth=2)
    if bvh == 2:
        assert violations(tracer) == []
    assert_same_floats(got, leaf_walk["frame"], "leaf walk frame, bvh=%d" % bvh)
    assert tracer.stats().fallback_frames == 0
    hits = tracer.trace_rays(leaf_walk["rays"], qs.RAY_REFLECTION)
    assert_same_records(hits, leaf_walk["want"], "leaf walk trace_rays, bvh=%d" % bvh)
    assert tracer.query_stats().rerouted == 0


@pytest.fixture(scope="module")
def ties(pkg, scenes, oracle):
    rays = rs.tie_rays()
    census = rs.tie_census(oracle, scenes, rays)
    assert all(int(census[k].sum()) >= 100 for k in "ABC"), {k: int(v.sum()) for k, v in census.items()}
    out = dict(rays=rays, census=census)
    for reverse in (False, True):
        scene, info = rs.tie_scene(reverse=reverse)
        o = oracle.OracleScene(scenes.to_blob(scene))
        out[reverse] = dict(scene=scene, info=info, frame=o.render(2)[0], want=qs.oracle_hits(o, scene, rays, qs.RAY_REFLECTION, pkg.HIT_DTYPE))
    return out


@pytest.mark.parametrize("bvh", [2, 1])
@pytest.mark.parametrize("reverse", [False, True], ids=["scene order", "reversed"])
def test_ties_go_to_the_references_winner(pkg, scenes, ties, reverse, bvh):
    """Coincident triangles (in one mesh: k3; as two objects: k2, seen in the colour; a BVH_TRI_WALK triangle: through
    bvh_leaf_walk): the frame and the records name the copy the reference names, in scene order and reversed."""
    c = ties[reverse]
    tracer = tracer_of(pkg, scenes, c["scene"], bvh=bvh)
    assert int(filter_note(tracer)["walk_triangles"]) >= 2
    got = tracer.render(max_depth=2)
    if bvh == 2:
        assert violations(tracer) == []
    assert_same_floats(got, c["frame"], "ties frame, reverse=%s bvh=%d" % (reverse, bvh))
    assert tracer.stats().fallback_frames == 0
    hits = tracer.trace_rays(ties["rays"], qs.RAY_REFLECTION)
    assert_same_records(hits, c["want"], "ties trace_rays, reverse=%s bvh=%d" % (reverse, bvh))
    if reverse:
        # the winner follows the scene's order: on the tied rays of kind B the winning OBJECT is the other copy (the other albedo)
        fwd, rev, tied = ties[False], ties[True], ties["census"]["B"]
        material = lambda c, h: np.array([o["material_index"] for o in c["scene"]["objects"]])[h["mesh"]]
        assert np.all(material(fwd, fwd["want"][tied]) != material(rev, hits[tied]))


# ---------------------------------------------------------------------------------------------------------------------- give_up
@pytest.fixture(scope="module")
def small_hw14(pkg, scenes, oracle):
    scene = mixed_scene(scenes)
    o = oracle.OracleScene(scenes.to_blob(scene))
    rays = rs.camera_rays(o)
    return dict(scene=scene, oracle=o, frame=o.render(MIXED_DEPTH)[0], rays=rays)


@pytest.mark.parametrize("tuning", [dict(), dict(level_queue=0)], ids=["defaults", "level_queue=0"])
def test_a_full_stack_sends_the_frame_to_the_last_resort(pkg, scenes, small_hw14, tuning):
    """Four stack entries on the small HW14 scene: walks give up, the frame is redone by the queue-less kernel (one fallback, the
    oracle's pixels), no walk reaches the spill buffer; with the built size back the next frame needs no fallback."""
    tracer = tracer_of(pkg, scenes, small_hw14["scene"], **tuning)
    tracer.set_filter_stack(4)
    before = tracer.stats().fallback_frames
    got = tracer.render(max_depth=MIXED_DEPTH)
    assert_same_floats(got, small_hw14["frame"], "small hw14 with 4 stack entries %r" % (tuning,))
    assert tracer.stats().fallback_frames == before + 1
    got = tracer.render(max_depth=MIXED_DEPTH, counters=2)
    mark = int(tracer.stream_counts()[SC_BVH_MARK])
    print("4 stack entries %r: high-water mark %d" % (tuning, mark))
    assert_same_floats(got, small_hw14["frame"], "small hw14 with 4 stack entries, tallying build")
    assert 0 < mark <= 4
    tracer.set_filter_stack(0xFFFFFFFF)
    before = tracer.stats().fallback_frames
    got = tracer.render(max_depth=MIXED_DEPTH)
    assert_same_floats(got, small_hw14["frame"], "small hw14, stack restored")
    assert tracer.stats().fallback_frames == before


def test_a_full_stack_reroutes_query_rays(pkg, scenes, small_hw14):
    tracer = tracer_of(pkg, scenes, small_hw14["scene"])
    tracer.set_filter_stack(4)
    rays, o, scene = small_hw14["rays"], small_hw14["oracle"], small_hw14["scene"]
    want = qs.oracle_hits(o, scene, rays, qs.RAY_REFLECTION, pkg.HIT_DTYPE)
    got = tracer.trace_rays(rays, qs.RAY_REFLECTION)
    assert_same_records(got, want, "trace_rays with 4 stack entries")
    assert 0 < tracer.query_stats().rerouted <= len(rays)
    want_occ = qs.oracle_occluded(o, rays, 6.0)
    got_occ = tracer.occluded_rays(rays, 6.0)
    assert np.array_equal(got_occ, want_occ)
    assert tracer.query_stats().rerouted > 0
    keep = ss.is_fixed_point(rays)
    assert keep.sum() > 100
    want_rgb, status_want = ss.oracle_colours(o, rays[keep]), ss.expected_status(pkg, scene, want[keep])
    rgb, status = tracer.shade_hits(want[keep])
    assert np.array_equal(status, status_want)
    exact = (status_want == pkg.SHADE_DIFFUSE) | (status_want == pkg.SHADE_BACKGROUND)
    assert_same_floats(rgb[exact], want_rgb[exact], "shade_hits with 4 stack entries")
    assert tracer.query_stats().rerouted > 0
