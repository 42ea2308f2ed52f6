"""Ill-formed triangles on the CPU (tests/degenerate_sets.py): the oracle against the real reference's frames of the four cases
(tests/golden/degenerate_*.npz), the route conditions that make those frames worth comparing -- NaN hits that win, the plane triangle
hit far outside its own box, shadow rays that test a zero-area triangle and are not occluded by it -- evaluated on the committed
fixtures, and what the host layer makes of such scenes: no candidate filter, the reference's normals."""
import ctypes as C

import numpy as np
import pytest

import degenerate_sets as ds
import query_sets as qs
from helpers import assert_same_floats, blob_to_scene, load_golden

TINY = np.float32(1e-25)


@pytest.mark.parametrize("case", ds.CASES)
def test_builder_makes_the_fixture(scenes, case):
    # the route conditions below are evaluated on degenerate_sets' scenes: they are the fixtures' scenes, byte for byte
    assert scenes.to_blob(ds.scene_of(scenes, case)[0]) == load_golden("degenerate_" + case)["blob"]
    assert load_golden("degenerate_" + case)["depth"] == ds.DEPTH


@pytest.mark.parametrize("case", ds.CASES)
def test_oracle_reproduces_reference_frame(scenes, oracle, case):
    g = load_golden("degenerate_" + case)
    assert_same_floats(ds.frame_of(scenes, oracle, case)[0], g["rgb"], case)
    got, _ = oracle.OracleScene(g["blob"]).render(g["depth"])          # and from the fixture's own blob
    assert_same_floats(got, g["rgb"], case + " (fixture blob)")


def test_ppm_bytes_with_nan_pixels(oracle, pkg, tmp_path):
    g = load_golden("degenerate_mixed")
    assert np.isnan(g["rgb"]).any()
    p1, p2 = str(tmp_path / "o.ppm"), str(tmp_path / "h.ppm")
    oracle.write_ppm(p1, g["rgb"])
    pkg.export_ppm(p2, g["rgb"])
    assert open(p1, "rb").read() == g["ppm"]                            # the x86 reference's own bytes (Color.cpp:12-21 on NaN)
    assert open(p2, "rb").read() == g["ppm"]


@pytest.fixture(scope="module")
def census(scenes, oracle):
    return {case: ds.route_census(scenes, oracle, case) for case in ds.CASES}


@pytest.mark.parametrize("case", ["zero", "mixed"])
def test_route_nan_pixels(census, case):
    # achieved: 22 (zero), 22 (mixed)
    g = load_golden("degenerate_" + case)
    assert int(ds.nan_pixels(g["rgb"]).sum()) >= 20 and census[case]["nan_pixels"] == int(ds.nan_pixels(g["rgb"]).sum())
    assert not ds.nan_pixels(load_golden("degenerate_plane")["rgb"]).any() and not ds.nan_pixels(load_golden("degenerate_needle")["rgb"]).any()


def test_route_plane_pixels(scenes, oracle, census):
    # achieved: 398; the reference's frame shows the plane too: those pixels differ from the frame of the scene without the triangle
    assert census["plane"]["plane_pixels"] >= 50
    g = load_golden("degenerate_plane")
    clean = ds.frame_of(scenes, oracle, "plane", bad=False)[0]
    assert int((g["rgb"].view(np.uint32) != clean.view(np.uint32)).any(axis=2).sum()) >= 50


@pytest.mark.parametrize("case", ["zero", "mixed"])
def test_route_shadow_rays_cross_a_zero_area_leaf_and_the_light_counts(census, case):
    # achieved: 468 (zero), 228 (mixed) floor pixels
    assert census[case]["shadow_crossings"] >= 20


def test_route_nan_winners_on_the_textured_meshes(scenes, census):
    # achieved: 8 on the checker mesh, 6 on the bitmap mesh, 8 on the mesh of its own
    _, marks = ds.scene_of(scenes, "mixed")
    winners = census["mixed"]["nan_winners"]
    assert winners.get(marks["zero_checker"][0], 0) >= 5 and winners.get(marks["zero_bitmap"][0], 0) >= 5
    zero = census["zero"]["nan_winners"]
    _, marks = ds.scene_of(scenes, "zero")
    assert zero.get(marks["zero_own"][0], 0) >= 5 and zero.get(marks["zero_mirror"][0], 0) >= 5   # 14 and 8: the smooth-shaded mesh wins too


def test_needle_is_hit_and_has_a_unit_normal(scenes, oracle):
    scene, marks = ds.scene_of(scenes, "needle")
    o = ds.oracle_of(scenes, oracle, "needle")
    mesh, _ = marks["needle"]
    _, hit, vals = ds.primary_hits(o)
    assert int((hit & (vals[:, 9] == mesh)).sum()) >= 10               # achieved: 21 pixels of row NEEDLE_ROW
    p = np.asarray(scene["objects"][mesh]["vertices"], dtype=np.float64)
    edges = sorted(np.linalg.norm(p[a] - p[b]) for a, b in ((0, 1), (1, 2), (2, 0)))
    assert edges[2] / edges[0] >= 1e4 * 0.99                            # 1 m x 0.1 mm
    fn, _ = o.mesh_normals(mesh)
    assert abs(float(np.linalg.norm(fn[0].astype(np.float64))) - 1.0) < 1e-6


def test_query_ray_set(scenes, oracle, pkg):
    rays = ds.query_rays(scenes, oracle)
    scene, _ = ds.scene_of(scenes, "mixed")
    o = ds.oracle_of(scenes, oracle, "mixed")
    assert len(rays["camera"]) == ds.W * ds.H and len(rays["reflection"]) >= 20 and len(rays["random"]) >= 200 and len(rays["shadow"]) >= 20
    hits = qs.oracle_hits(o, scene, rays["reflection"], qs.RAY_REFLECTION, pkg.HIT_DTYPE)
    assert qs.non_finite_winners(hits) >= 15                            # the reflection rays of the NaN pixels: most are NaN winners themselves
    assert not qs.oracle_occluded(o, rays["shadow"], rays["shadow_distance"]).all()


# ------------------------------------------------------------------------------------------------------------ the host layer
@pytest.mark.parametrize("case", ds.CASES)
def test_census_refuses_the_filter(pkg, scenes, case, tmp_path):
    """crt_bvh_census (the test library's host-only hook, as tests/golden/make_golden.py: has_filter uses it): a triangle without a
    usable margin -> no candidate filter for the scene; the same scene without the triangle has one."""
    L = pkg.lib()
    L.crt_bvh_census.argtypes = [C.POINTER(pkg.SceneDesc), C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 8)()
    for bad, want in ((True, pkg.CRT_ERR_INVALID), (False, pkg.CRT_OK)):
        scene, _ = ds.scene_of(scenes, case, bad=bad)
        hs = pkg.Scene(json_text=scenes.to_json(scene), folder=_folder(scenes, scene, tmp_path))
        assert L.crt_bvh_census(C.byref(hs.desc), out) == want, (case, bad)


@pytest.mark.parametrize("case", ds.CASES)
def test_host_stores_the_reference_normals(pkg, scenes, oracle, case, tmp_path):
    scene, marks = ds.scene_of(scenes, case)
    hs = pkg.Scene(json_text=scenes.to_json(scene), folder=_folder(scenes, scene, tmp_path))
    o = ds.oracle_of(scenes, oracle, case)
    assert hs.mesh_count == o.mesh_count
    for m in range(o.mesh_count):
        for got, want, what in zip(hs.mesh_normals(m), o.mesh_normals(m), ("face", "vertex")):
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (case, m, what)
    for name, (mesh, tri) in marks.items():
        fn, vn = hs.mesh_normals(mesh)
        if name.startswith("zero"):                                     # Vector.cpp:97-106: length 0 returns early
            assert np.array_equal(fn[tri].view(np.uint32), np.zeros(3, np.uint32)), name
            assert not np.any(vn[scene["objects"][mesh]["triangles"][tri]]), name   # vertices of no other triangle: the sum of nothing
        elif name == "plane":                                           # the squared length underflows: the cross product as it is
            assert np.array_equal(fn[tri], np.array([0, 0, TINY], dtype=np.float32)), fn[tri]
    # and the same trees, node for node
    for m in list(range(o.mesh_count)) + [-1]:
        for got, want in zip(hs.tree(m), o.tree(m)):
            assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), (case, m)


def _folder(scenes, scene, tmp_path):
    if not scene.get("textures"):
        return ""
    scenes.write_bitmaps(scene, str(tmp_path))
    return str(tmp_path)


def test_fixture_scene_survives_the_blob_round_trip(scenes):
    g = load_golden("degenerate_mixed")
    assert scenes.to_blob(blob_to_scene(g["blob"])) == g["blob"]        # the 1e-25 coordinate and the repeated vertex included
