"""The walk step of the filter kernels (csrc/kernel_bvh.h: bvh_step) fetches whatever its lane needs -- an inner node's record or a
leaf's next two triangles and their ids -- through ONE set of loads issued before the step branches on the lane's kind.  What can go
wrong with that: a lane consuming slots that were fetched for the other kind, a slot a lane does not need reading beyond its array
(the last filter entry, a leaf with one triangle left), and an index checked against the wrong array in the bounds-checked build.
The shapes are the smallest that reach each of these."""
import json
import os

import numpy as np
import pytest

from helpers import assert_same_floats

pytestmark = pytest.mark.gpu

SC_BVH_DIAG = 400        # csrc/kernel_bvh.h: the bounds-checked build's words in the frame's counter block, 16 (flag, index) pairs
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "walk_fetch_counts.json")


def tiny_scene(scenes, n_triangles):
    """One diffuse mesh of 1, 2 or 3 triangles facing the camera, one light in front of it.  The triangles are staggered in depth and
    overlap, so that the nearer ones shadow the farther ones: closest-hit walks and shadow walks both end in the mesh's leaf."""
    verts, tris = [], []
    for k in range(n_triangles):
        z = -3.0 - 0.4 * k
        x = -0.5 + 0.45 * k
        verts += [(x - 1.0, -0.8, z), (x + 1.0, -0.8, z), (x + 0.1, 0.9, z)]   # counter-clockwise seen from +z
        tris.append((3 * k, 3 * k + 1, 3 * k + 2))
    return {"settings": scenes._settings(32, 24),
            "camera": {"matrix": list(scenes.IDENTITY), "position": [0.0, 0.0, 0.0]},
            "lights": [{"intensity": 60, "position": [-1.5, 0.6, 0.5]}],
            "materials": [{"type": "diffuse", "albedo": [0.8, 0.6, 0.3], "smooth_shading": False}],
            "objects": [scenes._mesh(0, np.array(verts, dtype=np.float32), np.array(tris, dtype=np.uint32))]}


def mixed_scene(scenes):
    """The HW14 generator at its smallest detail (every tessellation count at its floor), 64x40: a room, a knot, a reflective and a
    refractive sphere -- level 0, the level queue and the bulk shadow pass all run waves that hold node lanes and leaf lanes."""
    return scenes.make("hw14", width=64, height=40, detail=0.005)


MIXED_DEPTH = 3


def tracer_of(pkg, scenes, scene, **tuning):
    return pkg.Tracer(pkg.Scene(json_text=scenes.to_json(scene)), tuning=pkg.make_tuning(**tuning) if tuning else None)


def violations(tracer):
    c = tracer.stream_counts()
    return [(k, int(c[SC_BVH_DIAG + 2 * k + 1])) for k in range(16) if c[SC_BVH_DIAG + 2 * k]]


@pytest.fixture(scope="module")
def tiny_frames(scenes, oracle):
    out = {}
    for n in (1, 2, 3):
        scene = tiny_scene(scenes, n)
        want, _ = oracle.OracleScene(scenes.to_blob(scene)).render(2)
        out[n] = (scene, want)
    return out


@pytest.fixture(scope="module")
def mixed_frame(scenes, oracle):
    scene = mixed_scene(scenes)
    want, _ = oracle.OracleScene(scenes.to_blob(scene)).render(MIXED_DEPTH)
    return scene, want


@pytest.mark.parametrize("bvh", [1, 2])
@pytest.mark.parametrize("n_triangles", [1, 2, 3])
def test_tiny_meshes_last_entry_and_single_triangle_leaf(pkg, scenes, tiny_frames, n_triangles, bvh):
    """A root whose children are leaves, a leaf whose only (or last) triangle is the LAST entry of bvh_tris / bvh_ids, and the leaf
    lane whose second triangle is the clamp case: the frame is the oracle's, no fallback, no recorded bounds violation."""
    scene, want = tiny_frames[n_triangles]
    assert (want != want[0, 0]).any()                      # the mesh is in the picture
    tracer = tracer_of(pkg, scenes, scene, bvh=bvh)
    assert tracer.kernels()["level0"].startswith("bvh_trace_")
    for frame in range(2):
        got = tracer.render(max_depth=2)
        assert_same_floats(got, want, "%d triangles, bvh=%d, frame %d" % (n_triangles, bvh, frame))
        assert tracer.stats().fallback_frames == 0
        if bvh == 2:
            assert violations(tracer) == []


@pytest.mark.parametrize("tuning", [dict(), dict(level_queue=0), dict(bvh=2), dict(level_queue=1 | (1 << 12))],
                         ids=["defaults", "level_queue=0", "bvh=2", "level_queue=4097"])
def test_mixed_waves_give_the_oracles_frame(pkg, scenes, mixed_frame, tuning):
    scene, want = mixed_frame
    tracer = tracer_of(pkg, scenes, scene, **tuning)
    assert tracer.kernels()["level0"].startswith("bvh_trace_")
    got = tracer.render(max_depth=MIXED_DEPTH)
    assert_same_floats(got, want, "small hw14 %r" % (tuning,))
    assert tracer.stats().fallback_frames == 0
    if tuning.get("bvh") == 2:
        assert violations(tracer) == []


def test_the_walk_executes_the_same_tests_as_before(pkg, scenes, mixed_frame):
    """The tallies of the tests the production kernels execute (collect_counters = 2) on the small HW14 frame equal the ones recorded
    from the kernels before the fetch was merged (tests/golden/walk_fetch_counts.json): a lane that consumed a record that was not
    its own would walk differently, even where the frame came out the same."""
    scene, want = mixed_frame
    golden = json.load(open(GOLDEN))
    assert golden["scene"] == {"generator": "hw14", "width": 64, "height": 40, "detail": 0.005, "max_depth": MIXED_DEPTH}
    tracer = tracer_of(pkg, scenes, scene)
    got = tracer.render(max_depth=MIXED_DEPTH, counters=2)
    assert_same_floats(got, want, "small hw14, tallying build")
    executed = tracer.executed_counters()
    print("executed:", executed)
    assert executed == golden["executed_counters"]
