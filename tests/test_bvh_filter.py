"""The candidate filter (csrc/crt_bvh.h, csrc/kernel_bvh.h) on the CPU: its hierarchy is built by the library's host code and its two
promises are checked against brute force by crt_bvh_selftest -- every triangle the reference's test accepts with a finite distance is
reached by the conservative walk; every triangle it accepts with an infinite or NaN distance in a leaf the ray's line passes is
reached by the miss check.  No GPU: the device kernels use the same expressions (tests/test_gpu_parity.py holds them to the oracle)."""
import ctypes as C

import numpy as np
import pytest

import query_sets as qs
import rare_sets as rs
from helpers import small_case


def _selftest(pkg, scenes, scene, rays, primary=False, folder=""):
    if scene.get("textures") and folder:
        scenes.write_bitmaps(scene, folder)
    hs = pkg.Scene(json_text=scenes.to_json(scene), folder=folder)
    L = pkg.lib()
    L.crt_bvh_selftest.argtypes = [C.POINTER(pkg.SceneDesc), C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 8)()
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    rc = L.crt_bvh_selftest(C.byref(hs.desc), rays.ctypes.data_as(C.c_void_p), len(rays), 1 if primary else 0, out)
    assert rc == 0
    return dict(zip(("rays", "finite_hits", "finite_missed", "other_hits", "other_missed", "nodes_1", "nodes_2", "errors"), [int(v) for v in out]))


def _random_rays(rng, n, lo, hi):
    o = rng.uniform(lo, hi, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], axis=1).astype(np.float32)


@pytest.mark.parametrize("name", ["hw08", "hw11", "hw14", "hw12"])
def test_filter_reaches_every_accepted_triangle(pkg, scenes, name, tmp_path):
    scene, _, _ = small_case(scenes, name)
    rng = np.random.default_rng(11)
    rays = _random_rays(rng, 300, [-3.5, -2.0, -8.5], [3.5, 3.0, 1.5])       # in and around the room, any direction
    r = _selftest(pkg, scenes, scene, rays, folder=str(tmp_path))
    assert r["errors"] == 0
    assert r["finite_hits"] > (200 if name != "hw08" else 50) and r["finite_missed"] == 0     # (some origins lie outside the room, and hw08 is no room at all)
    assert r["other_missed"] == 0
    assert r["nodes_1"] < 0.2 * r["finite_hits"] * 400                         # a walk, not a sweep of the hierarchy


def test_rays_parallel_to_planes_are_seen_by_the_miss_check(pkg, scenes):
    """Directions with exact zeros: d . n is exactly 0 for the room's walls, the reference's test divides by it, and whatever it then
    accepts (infinite and NaN distances) must be among what the miss check reaches -- and zero components must not turn the
    conservative walk into a sweep."""
    scene, _, _ = small_case(scenes, "hw11")
    rng = np.random.default_rng(5)
    rays = []
    for axis in range(3):
        for _ in range(60):
            o = rng.uniform([-2.9, -1.4, -7.9], [2.9, 2.4, 0.9])
            d = rng.normal(size=3)
            d[axis] = 0.0
            d /= np.linalg.norm(d)
            rays.append(np.concatenate([o, d]))
        for sign in (1.0, -1.0):                                               # along an axis: two zero components
            d = np.zeros(3)
            d[axis] = sign
            rays.append(np.concatenate([rng.uniform([-2.9, -1.4, -7.9], [2.9, 2.4, 0.9]), d]))
    # origins ON the walls' planes, directions in them: the numerator is zero too (0 / 0)
    rays.append([-3.0, 0.0, -4.0, 0.0, 0.6, -0.8])
    rays.append([0.5, -1.5, -3.0, 0.6, 0.0, -0.8])
    r = _selftest(pkg, scenes, scene, np.array(rays))
    assert r["errors"] == 0 and r["finite_missed"] == 0 and r["other_missed"] == 0
    assert r["other_hits"] > 0                                                 # the case exists: some of these rays are "hit" at infinity
    assert r["nodes_2"] < len(rays) * 400


def test_primary_rays_of_the_benchmark_scene(pkg, scenes):
    scene = scenes.make("hw14", width=64, height=36, detail=0.2)               # ~8k triangles
    cam = np.array(scene["camera"]["position"], dtype=np.float32)
    rng = np.random.default_rng(3)
    d = np.stack([rng.uniform(-0.9, 0.9, 200), rng.uniform(-0.5, 0.5, 200), -np.ones(200)], axis=1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([np.tile(cam, (200, 1)), d], axis=1)
    r = _selftest(pkg, scenes, scene, rays, primary=True)
    assert r["errors"] == 0 and r["finite_hits"] >= 200 and r["finite_missed"] == 0 and r["other_missed"] == 0


# ---- the scenes of the rare routes (tests/rare_sets.py; the GPU side is tests/test_gpu_filter_rare.py)
def _census(pkg, scenes, scene):
    hs = pkg.Scene(json_text=scenes.to_json(scene))
    L = pkg.lib()
    L.crt_bvh_census.argtypes = [C.POINTER(pkg.SceneDesc), C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 8)()
    assert L.crt_bvh_census(C.byref(hs.desc), out) == 0
    return dict(zip(("nodes", "entries", "depth", "wide_depth", "walk_triangles"), [int(v) for v in out]))


def _assert_filter_holds(r, n_rays):
    assert r["errors"] == 0 and r["finite_missed"] == 0 and r["other_missed"] == 0
    assert r["finite_hits"] > n_rays // 2


def test_deep_stack_scene_census(pkg, scenes, oracle):
    """The filter of the card scene is deep enough for its walks to outgrow the 16 stack entries held in LDS, first hits land at
    every depth of the stack of cards, deeper levels and shadow rays exist, and the filter's two promises hold for the ray set
    (every sixteenth ray: the brute force behind the self-test is rays x cards)."""
    scene = rs.deep_stack_scene()
    c = _census(pkg, scenes, scene)
    print("deep stack: n %d census %r" % (rs.DEEP_N, c))
    assert 3 * c["wide_depth"] + 1 > 16 and c["entries"] == rs.DEEP_N and c["walk_triangles"] == 0
    # six levels of four children each: a walk along the line holds up to 18 entries.  Half as many cards: one level has two children,
    # 3 x 5 + 1 = 16 entries, all in LDS (measured on the GPU: 16)
    assert (c["depth"], c["wide_depth"]) == (12, 6) and c["nodes"] == (4 ** 6 - 1) // 3
    half = _census(pkg, scenes, rs.deep_stack_scene(rs.DEEP_N // 2))
    assert (half["depth"], half["wide_depth"]) == (11, 6)
    o = oracle.OracleScene(scenes.to_blob(scene))
    rays = rs.deep_stack_rays(o)
    assert len(rays) == 2 * 32 * 24 + 2048
    frame, counters = o.render(3)
    assert len(np.unique(frame.reshape(-1, 3), axis=0)) > 300          # a hit's colour says which card it was
    hits = qs.oracle_hits(o, scene, rays, qs.RAY_REFLECTION, pkg.HIT_DTYPE)
    cards = rs.first_hit_cards(scene, hits)
    quartiles = np.quantile(cards[cards >= 0], [0.25, 0.5, 0.75])
    print("deep stack: hits %d of %d, first-hit card quartiles %r" % (int(hits["hit"].sum()), len(rays), quartiles))
    assert quartiles[0] < rs.DEEP_N // 4 and quartiles[2] > rs.DEEP_N // 2
    mirrors = hits["hit"].astype(bool) & (hits["mesh"] == 1)
    assert mirrors.sum() > 200                                           # reflection children
    _assert_filter_holds(_selftest(pkg, scenes, scene, rays[::16]), len(rays[::16]))


def test_leaf_walk_scene_census(pkg, scenes, oracle):
    scene, large = rs.leaf_walk_scene()
    assert _census(pkg, scenes, scene)["walk_triangles"] >= 2
    o = oracle.OracleScene(scenes.to_blob(scene))
    rays = rs.leaf_walk_rays()
    hits = qs.oracle_hits(o, scene, rays, qs.RAY_REFLECTION, pkg.HIT_DTYPE)
    share_large, share_in_front = rs.leaf_walk_census(scene, large, rays, hits)
    print("leaf walk: winners %d, large %.3f, small in front of a large one %.3f" % (int(hits["hit"].sum()), share_large, share_in_front))
    assert share_large >= 0.2 and share_in_front >= 0.2
    assert len(np.unique(hits["mesh"][hits["hit"].astype(bool)])) == 2  # cache_mesh changes along rays
    _assert_filter_holds(_selftest(pkg, scenes, scene, rays), len(rays))


def test_tie_scene_census(pkg, scenes, oracle):
    """At least 100 rays per kind on which both copies are hit at the same bit pattern of t; the reversed scene names the other copy."""
    rays = rs.tie_rays()
    census = rs.tie_census(oracle, scenes, rays)
    print("ties:", {k: int(v.sum()) for k, v in census.items()})
    assert all(int(census[k].sum()) >= 100 for k in "ABC")
    winners = {}
    for reverse in (False, True):
        scene, info = rs.tie_scene(reverse=reverse)
        assert _census(pkg, scenes, scene)["walk_triangles"] >= 2
        o = oracle.OracleScene(scenes.to_blob(scene))
        hits = qs.oracle_hits(o, scene, rays, qs.RAY_REFLECTION, pkg.HIT_DTYPE)
        material = np.array([ob["material_index"] for ob in scene["objects"]])[hits["mesh"]]
        winners[reverse] = material[census["B"]]
        _assert_filter_holds(_selftest(pkg, scenes, scene, rays), len(rays))
    assert set(winners[False]) == {1} and set(winners[True]) == {2}     # the first copy in the scene's order, whichever it is
