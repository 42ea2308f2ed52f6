"""Direct lighting for the caller's records (include/crt_hip.h: crt_shade_hits*, crt_light_points*), what needs no GPU: the constants
and bindings against the header, and that the record sets of tests/test_gpu_shade_hits.py are what that file takes them for --
checked with the oracle alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import query_sets as qs
import shade_sets as ss
from helpers import assert_same_floats, small_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["crt_shade_hits", "crt_shade_hits_device", "crt_light_points", "crt_light_points_device"]
# the oracle's census of the fixed-point subset of query_sets.random_rays() per scene (misses, diffuse, reflective, refractive hits;
# diffuse hits with some / all lights occluded)
CENSUS = {
    "hw08": dict(misses=2087, diffuse=1212, reflective=0, refractive=0, partly=410, wholly=19),
    "hw11": dict(misses=969, diffuse=2170, reflective=81, refractive=79, partly=300, wholly=4),
    "hw12": dict(misses=970, diffuse=2238, reflective=54, refractive=37, partly=761, wholly=31),
    "hw14": dict(misses=969, diffuse=2276, reflective=28, refractive=26, partly=741, wholly=98),
}


def header():
    return open(os.path.join(ROOT, "include", "crt_hip.h")).read()


def test_constants_and_layouts_match_the_header(pkg):
    m = re.search(r"enum \{ CRT_SHADE_BACKGROUND = (\d), CRT_SHADE_DIFFUSE = (\d), CRT_SHADE_RECURSES = (\d), CRT_SHADE_INVALID = (\d) \};", header())
    assert m, "the CRT_SHADE_* enum is not in include/crt_hip.h"
    assert tuple(int(x) for x in m.groups()) == (pkg.SHADE_BACKGROUND, pkg.SHADE_DIFFUSE, pkg.SHADE_RECURSES, pkg.SHADE_INVALID) == (0, 1, 2, 3)
    # the records are crt_trace_rays' (48 bytes), the options crt_render's (shadow_bias at 4, use_gi at 16)
    assert C.sizeof(pkg.Hit) == 48 == pkg.HIT_DTYPE.itemsize and C.sizeof(pkg.Options) == 40
    assert (pkg.Options.shadow_bias.offset, pkg.Options.use_gi.offset) == (4, 16)
    L = pkg.lib()
    vp = C.c_void_p
    assert L.crt_shade_hits.argtypes == [vp, vp, C.c_uint64, C.POINTER(pkg.Options), vp, vp]
    assert L.crt_shade_hits_device.argtypes == [vp, vp, C.c_uint64, C.POINTER(pkg.Options), vp, vp, vp]
    assert L.crt_light_points.argtypes == [vp, vp, vp, C.c_uint64, C.c_float, vp]
    assert L.crt_light_points_device.argtypes == [vp, vp, vp, C.c_uint64, C.c_float, vp, vp]


def test_shade_symbols_are_declared_and_exported(pkg):
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    plain = C.CDLL(os.path.join(os.path.dirname(pkg.LIB_PATH), "libcrt_hip.so"))
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, text), name + " is not declared"
        assert name in pkg.DEVICE_SYMBOLS and hasattr(pkg.lib(), name) and hasattr(plain, name), name
    for method in ("shade_hits", "light_points", "shade_hits_device", "light_points_device"):
        assert callable(getattr(pkg.Tracer, method))


def test_fixed_point_rays_are_what_shoot_ray_leaves_alone(pkg):
    rays = qs.random_rays()
    keep = ss.is_fixed_point(rays)
    assert int(keep.sum()) == 3299 and len(rays) == 4096
    fp = ss.fixed_point_rays(rays)
    assert fp.shape == (3299, 6) and fp.dtype == np.float32
    # Vector::normalize in float32 returns these directions bit for bit -- and changes at least one of the others
    assert_same_floats(ss.normalized_like_shoot_ray(fp), fp[:, 3:], "fixed points")
    rest = rays[~keep]
    assert np.any(ss.normalized_like_shoot_ray(rest).view(np.uint32) != rest[:, 3:].view(np.uint32))
    assert pkg.SHADE_DIFFUSE == 1


@pytest.mark.parametrize("name", ["hw08", "hw11", "hw12", "hw14"])
def test_the_random_set_s_census(pkg, scenes, oracle, name):
    """What the GPU tests rely on: the set has misses, diffuse hits in light, in part shadow and in full shadow, and (hw11, hw12, hw14)
    hits that recurse -- by the oracle, at least 1200 diffuse records and 300 partly shadowed ones in every scene."""
    scene, _, _ = small_case(scenes, name)
    o = oracle.OracleScene(scenes.to_blob(scene))
    rays = ss.fixed_point_rays(qs.random_rays())
    hits = qs.oracle_hits(o, scene, rays, qs.RAY_REFLECTION, pkg.HIT_DTYPE)
    got = ss.census(pkg, o, scene, hits)
    print(name, got)
    assert got == CENSUS[name]
    assert got["diffuse"] >= 1200 and got["partly"] >= 300
    status = ss.expected_status(pkg, scene, hits)
    assert int((status == pkg.SHADE_DIFFUSE).sum()) == got["diffuse"]
    assert int((status == pkg.SHADE_RECURSES).sum()) == got["reflective"] + got["refractive"]
    assert int((status == pkg.SHADE_BACKGROUND).sum()) == got["misses"]


def test_white_scene_has_equal_channels(pkg, scenes, oracle):
    scene, _, _ = small_case(scenes, "hw12")
    white = ss.white_scene(scene)
    assert "textures" not in white and "textures" in scene
    assert all(m["albedo"] == [1.0, 1.0, 1.0] for m in white["materials"] if m["type"] == "diffuse")
    assert [m["type"] for m in white["materials"]] == [m["type"] for m in scene["materials"]]
    assert white["lights"] == scene["lights"] and len(white["objects"]) == len(scene["objects"])
    o = oracle.OracleScene(scenes.to_blob(white))
    rays = ss.fixed_point_rays(qs.random_rays(512))
    hits = qs.oracle_hits(o, white, rays, qs.RAY_REFLECTION, pkg.HIT_DTYPE)
    diffuse = ss.expected_status(pkg, white, hits) == pkg.SHADE_DIFFUSE
    rgb = ss.oracle_colours(o, rays)[diffuse]
    assert len(rgb) > 100 and np.any(rgb > 0)
    assert_same_floats(rgb[:, 1], rgb[:, 0], "green")
    assert_same_floats(rgb[:, 2], rgb[:, 0], "blue")


def test_in_plane_set_has_diffuse_records_at_no_finite_point(pkg, scenes, oracle):
    """The reroute door of the GPU test: in-plane rays whose winner lies at t = inf / NaN on a DIFFUSE mesh exist."""
    scene, _, _ = small_case(scenes, "hw11")
    o = oracle.OracleScene(scenes.to_blob(scene))
    rays = ss.fixed_point_rays(qs.in_plane_rays(scene))
    hits = qs.oracle_hits(o, scene, rays, qs.RAY_REFLECTION, pkg.HIT_DTYPE)
    status = ss.expected_status(pkg, scene, hits)
    bad_point = ~np.isfinite(hits["point"]).all(axis=1)
    n = int(((status == pkg.SHADE_DIFFUSE) & bad_point).sum())
    print("in-plane hw11 fixed points: %d rays, %d diffuse records with a non-finite point" % (len(rays), n))
    assert len(rays) > 1000 and n > 0


def test_recorded_shade_times_are_complete():
    """profiles/shade_hits.json (tools/shade_time.py on an MI355X; no threshold: nobody had measured this): the queries' numbers on the
    frame's own records beside the parent commit's depth-0 frame, re-measured on the same machine."""
    import json
    doc = json.load(open(os.path.join(ROOT, "profiles", "shade_hits.json")))
    q, frame = doc["queries"], doc["frame"]
    assert q["repeats"] >= 20 and q["warmup"] >= 5 and frame["repeats"] >= 20 and frame["commit"] and q["csrc_sha256"] != frame["csrc_sha256"]
    n = 1920 * 1080
    s = q["s_shade_hits"]
    assert s["records"] == n == q["t_trace_camera_rays"]["records"]
    assert sum(q["status_counts"]) == n and q["status_counts"][1] == s["diffuse"] > n // 2 and q["status_counts"][3] == 0
    assert q["p_light_points"]["records"] == q["p_light_points"]["diffuse"] == n - q["status_counts"][0]
    assert q["s0_shade_hits_reference_order_kernel_alone"]["rerouted"] == s["diffuse"]
    for k in ("t_trace_camera_rays", "s_shade_hits", "p_light_points", "ts_trace_then_shade"):
        assert q[k]["ms"] > 0
    assert frame["depth0_frame_ms"] > 0 and q["depth0_frame_ms"] > 0
