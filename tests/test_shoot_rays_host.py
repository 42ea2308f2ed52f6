"""Radiance queries (include/crt_hip.h: crt_shoot_rays*), what needs no GPU: the bindings and the statistics' layout against the header
and the compiled library, and that the ray sets of tests/test_gpu_shoot_rays.py are what that file takes them for -- checked with the
oracle alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import query_sets as qs
import shoot_sets as sh
from helpers import small_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["crt_shoot_rays", "crt_shoot_rays_device", "crt_get_shoot_stats"]
# per scene: rays of shoot_sets.rays_for, and how many of them meet a mirror or glass mesh first (by the oracle)
CENSUS = {"hw08": (4096, 0), "hw11": (4096, 207), "hw12": (4096, 110), "hw14": (4480, 266)}


def header():
    return open(os.path.join(ROOT, "include", "crt_hip.h")).read()


def test_shoot_stats_layout_matches_the_compiled_library(pkg):
    offsets = (C.c_uint32 * 6)()
    size = pkg.lib().crt_host_shoot_stats_layout(offsets, 6)
    S = pkg.ShootStats
    assert size == C.sizeof(S) == 8 + 4 + 4 + 64 * 8 + 8 + 8 + 8
    assert list(offsets) == [S.rays.offset, S.levels.offset, S.level_rays.offset, S.shadow_records.offset, S.rerouted.offset, S.kernel_ms.offset]
    assert list(offsets) == [0, 8, 16, 528, 536, 544]
    # the header's struct, field for field
    m = re.search(r"typedef struct crt_shoot_stats \{(.*?)\} crt_shoot_stats;", header(), flags=re.S)
    assert m, "crt_shoot_stats is not in include/crt_hip.h"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [re.sub(r"\s+", " ", f.strip()) for f in body.split(";") if f.strip()]
    assert fields == ["uint64_t rays", "uint32_t levels", "uint32_t pad", "uint64_t level_rays[64]", "uint64_t shadow_records",
                      "uint64_t rerouted", "double kernel_ms"]
    assert [n for n, _ in S._fields_] == [f.split(" ")[1].split("[")[0] for f in fields]
    assert C.sizeof(pkg.Ray) == 24 and C.sizeof(pkg.Options) == 40
    assert [getattr(pkg.Options, k).offset for k in ("max_depth", "shadow_bias", "reflection_bias", "refraction_bias", "use_gi")] == [0, 4, 8, 12, 16]


def test_shoot_symbols_are_declared_and_exported(pkg):
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    plain = C.CDLL(os.path.join(os.path.dirname(pkg.LIB_PATH), "libcrt_hip.so"))
    L = pkg.lib()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, text), name + " is not declared"
        assert name in pkg.DEVICE_SYMBOLS and hasattr(L, name) and hasattr(plain, name), name
    assert "crt_host_shoot_stats_layout" in pkg.HOST_SYMBOLS and hasattr(plain, "crt_host_shoot_stats_layout")
    vp = C.c_void_p
    assert L.crt_shoot_rays.argtypes == [vp, vp, C.c_uint64, C.c_uint32, C.POINTER(pkg.Options), vp]
    assert L.crt_shoot_rays_device.argtypes == [vp, vp, C.c_uint64, C.c_uint32, C.POINTER(pkg.Options), vp, vp]
    assert L.crt_get_shoot_stats.argtypes == [vp, C.POINTER(pkg.ShootStats)]
    for method in ("shoot_rays", "shoot_rays_device", "shoot_stats"):
        assert callable(getattr(pkg.Tracer, method))
    # the header says what a caller of the device variant has to know
    contract = header()
    assert "ONCE PER LEVEL" in contract and "CANNOT BE CAPTURED INTO A hipGraph" in contract


def test_builders_are_deterministic(pkg, scenes):
    scene, _, _ = small_case(scenes, "hw14")
    a, b = sh.aimed_rays(scene), sh.aimed_rays(scene)
    assert a.dtype == np.float32 and a.shape == (384, 6) and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    lengths = np.linalg.norm(a[:, 3:].astype(np.float64), axis=1)
    assert lengths.min() > 0.1 and lengths.max() > 2.0, "the aimed directions are differences of points: not unit vectors"
    rays = sh.rays_for("hw14", scene)
    assert np.array_equal(rays[:4096], qs.random_rays()) and np.array_equal(rays[4096:], a)
    shaped = sh.shaped_rays(scene)
    assert shaped.shape == (4096, 6) and np.array_equal(shaped[:384], a) and np.array_equal(shaped[384:], qs.random_rays()[:4096 - 384])
    hw08, _, _ = small_case(scenes, "hw08")
    assert sh.aimed_rays(hw08).shape == (0, 6), "a scene without mirror or glass meshes has no aimed rays"
    assert np.array_equal(sh.rays_for("hw11", scene), qs.random_rays())
    # normalized_rays: Vector::normalize in float32, a zero direction left alone
    odd = np.array([[0, 0, 0, 0, 0, 0], [1, 2, 3, 0, 3, 4]], dtype=np.float32)
    assert np.array_equal(sh.normalized_rays(odd), np.array([[0, 0, 0, 0, 0, 0], [1, 2, 3, 0, np.float32(3) * (np.float32(1) / np.float32(5)),
                                                                                  np.float32(4) * (np.float32(1) / np.float32(5))]], dtype=np.float32))


@pytest.mark.parametrize("name", ["hw08", "hw11", "hw12", "hw14"])
def test_the_sets_are_not_empty_cases(pkg, scenes, oracle, name):
    """What the GPU tests rely on: on hw11 and hw14 at least 100 rays of the set meet a mirror or glass mesh first, and the colours
    change between max_depth 1 and 2 -- some ray of level 1 recurses again, so level 2 holds rays."""
    scene, depth, _ = small_case(scenes, name)
    o = oracle.OracleScene(scenes.to_blob(scene))
    rays = sh.rays_for(name, scene)
    got = (len(rays), sh.recursing_first_hits(pkg, o, scene, rays))
    print(name, got)
    assert got == CENSUS[name]
    if name in ("hw11", "hw14"):
        assert got[1] >= 100 and sh.level_two_matters(o, rays) and depth >= 2
    if name == "hw14":
        assert sh.recursing_first_hits(pkg, o, scene, qs.random_rays()) < 100, "why the aimed rays are there"
        assert sh.recursing_first_hits(pkg, o, scene, sh.shaped_rays(scene)[:63]) >= 10 and sh.level_two_matters(o, sh.shaped_rays(scene)[:512])
    if name == "hw08":
        assert not sh.level_two_matters(o, rays)


def test_in_plane_rays_have_nan_colours(pkg, scenes, oracle):
    scene, depth, _ = small_case(scenes, "hw11")
    o = oracle.OracleScene(scenes.to_blob(scene))
    want = sh.oracle_colours(o, qs.in_plane_rays(scene), depth)
    assert int(np.isnan(want).any(axis=1).sum()) > 100


def test_recorded_shoot_times_are_complete():
    """profiles/shoot_rays.json (tools/shoot_time.py on an MI355X; no threshold: the level-synchronous form is expected to be slower than
    the frame, and the file records by how much): the radiance queries on the frame's own camera rays at three depths and on random
    rays, beside the parent commit's frame of the same camera and depth, measured in the same session."""
    import json
    doc = json.load(open(os.path.join(ROOT, "profiles", "shoot_rays.json")))
    q, frame = doc["queries"], doc["frame"]
    assert q["repeats"] >= 20 and q["warmup"] >= 5 and frame["repeats"] >= 20 and frame["commit"]
    n = 1920 * 1080
    for depth in (0, 5, 8):
        row = q["camera_rays"][str(depth)]
        assert row["rays"] == n and row["ms"] > 0 and row["levels"] <= depth + 1 and row["level_rays"][0] == n
        assert frame["frame_ms"][str(depth)] > 0 and q["frame_ms"][str(depth)] > 0
    assert q["random_rays"]["rays"] == n and q["random_rays"]["ms"] > 0 and q["random_rays"]["max_depth"] == 8
