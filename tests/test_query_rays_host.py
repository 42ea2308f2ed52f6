"""Ray queries (include/crt_hip.h: crt_trace_rays*, crt_occluded_rays*), what needs no GPU: the records' layout, and that the ray sets
of tests/test_gpu_query_rays.py go where they are meant to go -- checked with the oracle alone."""
import ctypes as C

import numpy as np
import pytest

import query_sets as qs
from helpers import small_case


def test_record_layouts_match_the_header(pkg):
    assert C.sizeof(pkg.Ray) == 24 and C.sizeof(pkg.Hit) == 48 and C.sizeof(pkg.QueryStats) == 32
    assert (pkg.Ray.origin.offset, pkg.Ray.direction.offset) == (0, 12)
    want = dict(t=0, point=4, normal=16, u=28, v=32, mesh=36, triangle=40, hit=44)
    assert {k: getattr(pkg.Hit, k).offset for k in want} == want
    assert pkg.HIT_DTYPE.itemsize == 48 and {k: pkg.HIT_DTYPE.fields[k][1] for k in want} == want
    assert (pkg.RAY_PRIMARY, pkg.RAY_SHADOW, pkg.RAY_REFLECTION, pkg.RAY_REFRACTION) == (0, 1, 2, 3)     # enum RayType, Ray.h:14
    assert {k: getattr(pkg.QueryStats, k).offset for k in ("rays", "hits", "rerouted", "kernel_ms")} == dict(rays=0, hits=8, rerouted=16, kernel_ms=24)


def test_query_symbols_are_declared_and_exported(pkg):
    names = ["crt_trace_rays", "crt_trace_rays_device", "crt_occluded_rays", "crt_occluded_rays_device", "crt_camera_rays_device",
             "crt_get_query_stats"]
    for name in names:
        assert name in pkg.DEVICE_SYMBOLS and hasattr(pkg.lib(), name), name


def test_in_plane_rays_are_hits_at_no_finite_distance(pkg, scenes, oracle):
    """A cap on the in-plane set: at least 100 of its 1800 rays must be, by the oracle, a hit with a non-finite t when the ray is not
    a primary one (and none when it is: Ray.cpp:13 rejects d . n >= 0) -- or the GPU test could pass without a single refuted miss."""
    scene, _, _ = small_case(scenes, "hw11")
    rays = qs.in_plane_rays(scene)
    assert rays.shape == (1800, 6) and rays.dtype == np.float32
    assert np.all(np.abs(np.linalg.norm(rays[:, 3:].astype(np.float64), axis=1) - 1) < 1e-6)
    o = oracle.OracleScene(scenes.to_blob(scene))
    refl = qs.oracle_hits(o, scene, rays, qs.RAY_REFLECTION, pkg.HIT_DTYPE)
    prim = qs.oracle_hits(o, scene, rays, qs.RAY_PRIMARY, pkg.HIT_DTYPE)
    print("in-plane hw11: reflection hits %d non-finite %d; primary hits %d non-finite %d" % (
        int(refl["hit"].sum()), qs.non_finite_winners(refl), int(prim["hit"].sum()), qs.non_finite_winners(prim)))
    assert qs.non_finite_winners(refl) >= 100
    assert qs.non_finite_winners(prim) == 0 and int(prim["hit"].sum()) > 0


@pytest.mark.parametrize("name", ["hw08", "hw11", "hw14"])
def test_random_rays_have_finite_winners(pkg, scenes, oracle, name):
    """The random set's winners are finite on these scenes: the GPU test may ask for rerouted == 0."""
    scene, _, _ = small_case(scenes, name)
    hits = qs.oracle_hits(oracle.OracleScene(scenes.to_blob(scene)), scene, qs.random_rays(), qs.RAY_REFLECTION, pkg.HIT_DTYPE)
    print("random %s: hits %d non-finite %d" % (name, int(hits["hit"].sum()), qs.non_finite_winners(hits)))
    assert int(hits["hit"].sum()) > 1000 and qs.non_finite_winners(hits) == 0


def test_triangle_bases_follow_the_flattened_scene(pkg, scenes):
    scene, _, _ = small_case(scenes, "hw11")
    hs = pkg.Scene(json_text=scenes.to_json(scene))
    bases = qs.triangle_bases(scene)
    total = sum(len(np.asarray(o["triangles"]).reshape(-1, 3)) for o in scene["objects"])
    assert hs.desc.n_triangles == total and len(bases) == hs.desc.n_meshes and bases[0] == 0
    # the first triangle of every object in the flattened array is that object's first triangle: same first vertex
    tris = hs.desc.triangles
    for m, o in enumerate(scene["objects"]):
        v = np.asarray(o["vertices"], dtype=np.float32).reshape(-1, 3)[np.asarray(o["triangles"]).reshape(-1, 3)[0][0]]
        assert tuple(tris[int(bases[m])].v0) == tuple(v)


def test_recorded_query_times_hold_the_issue_s_condition():
    """profiles/query_rays.json (tools/query_time.py on an MI355X): closest hits of the frame's own camera rays take no longer than the
    parent commit's whole depth-0 frame of the same scene and camera, which walks those rays and then shades them."""
    import json
    import os
    doc = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "query_rays.json")))
    q, frame = doc["queries"], doc["frame"]
    assert q["repeats"] >= 20 and frame["repeats"] >= 20 and frame["commit"] and q["csrc_sha256"] != frame["csrc_sha256"]
    a = q["a_camera_rays_closest"]
    assert a["rays"] == 1920 * 1080 and a["rerouted"] == 0
    assert a["ms"] <= frame["depth0_frame_ms"]
    assert q["a0_camera_rays_closest_reroute_kernel_alone"]["rerouted"] == a["rays"]
