"""The candidate filter (csrc/crt_bvh.cpp, csrc/kernel_bvh.h) on the CPU, away from unit scale and away from the origin: the scenes and
ray sets of tests/scale_sets.py through crt_bvh_selftest (see tests/test_bvh_filter.py), and the conditions that keep those sets from
being vacuous, computed with the oracle alone.  No GPU: tests/test_gpu_scale.py is the device side.

What each set is for:
    room   the rays of every other test, through the same transform
    far    origins 1e2 .. 1e6 extents away: rho = 2^-16 (extent + |origin|) must cover the rounding of a hit point that far out
    rim    hit points ON the rim of the triangles' acceptance regions: only the margin added to the boxes (triangle_margin) lets
           the walk reach a triangle whose accepted point lies outside it -- where rho does not hide the margin, i.e. at small scale
"""
import ctypes as C

import numpy as np
import pytest

import query_sets as qs
import scale_sets as sc


def census(pkg, scenes, scene):
    """crt_bvh_census: None when the library says the scene has no filter"""
    hs = pkg.Scene(json_text=scenes.to_json(scene))
    L = pkg.lib()
    L.crt_bvh_census.argtypes = [C.POINTER(pkg.SceneDesc), C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 8)()
    rc = L.crt_bvh_census(C.byref(hs.desc), out)
    assert rc in (pkg.CRT_OK, pkg.CRT_ERR_INVALID)
    return dict(zip(("nodes", "entries", "depth", "wide_depth", "walk_triangles"), [int(v) for v in out])) if rc == pkg.CRT_OK else None


def selftest(pkg, scenes, scene, rays):
    hs = pkg.Scene(json_text=scenes.to_json(scene))
    L = pkg.lib()
    L.crt_bvh_selftest.argtypes = [C.POINTER(pkg.SceneDesc), C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 8)()
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    assert L.crt_bvh_selftest(C.byref(hs.desc), rays.ctypes.data_as(C.c_void_p), len(rays), 0, out) == 0
    return dict(zip(("rays", "finite_hits", "finite_missed", "other_hits", "other_missed", "nodes_1", "nodes_2", "errors"), [int(v) for v in out]))


def has_filter(base, case):
    return case != "lo"


@pytest.mark.parametrize("base", list(sc.BASES))
def test_the_bracket_has_not_moved(pkg, scenes, base):
    """tests/golden/scale_cases.json holds the two scales around the loss of the filter, by the library's own verdict.  A moved bracket
    means the margin rule (triangle_margin) changed: regenerate the fixture on purpose (tests/golden/make_golden.py scale)."""
    b = sc.bracket(base)
    assert 1.0 < b["S_hi"] / b["S_lo"] <= 1.25
    hi, lo = sc.make_case(scenes, base, "hi"), sc.make_case(scenes, base, "lo")
    assert census(pkg, scenes, hi) is not None, "the scene has lost its filter at S_hi"
    assert census(pkg, scenes, lo) is None, "the scene has a filter at S_lo"
    assert sc.shortest_edge(hi) == pytest.approx(b["shortest_edge_hi"], rel=1e-6) and sc.shortest_edge(lo) == pytest.approx(b["shortest_edge_lo"], rel=1e-6)
    # what the rule says at these sizes: the test's tolerance FLT_EPSILON over an edge of 1e-3 is a tenth of that edge
    assert 5e-4 < b["shortest_edge_lo"] < b["shortest_edge_hi"] < 2e-3
    assert scenes.triangle_count(hi) == b["triangles"]


@pytest.mark.parametrize("base,case", sc.all_cases() + [sc.EXCLUDED])
def test_which_cases_have_a_filter(pkg, scenes, base, case):
    """Every case of the grid but S_lo has a filter -- the case at s = 1e6 too: the filter does not refuse a scene for its size."""
    assert (census(pkg, scenes, sc.make_case(scenes, base, case)) is not None) == has_filter(base, case)


@pytest.mark.parametrize("base,case", [bc for bc in sc.all_cases() if has_filter(*bc)] + [sc.EXCLUDED])
def test_filter_reaches_every_accepted_triangle(pkg, scenes, oracle, base, case):
    d = sc.case_data(pkg, scenes, oracle, base, case)
    for name in ("room", "far", "rim"):
        rays = d[name]
        r = selftest(pkg, scenes, d["scene"], rays)
        print("%s %s %s: %r, nodes per finite hit %.1f" % (base, case, name, r, r["nodes_1"] / max(1, r["finite_hits"])))
        assert r["rays"] == len(rays) <= 2048 and r["errors"] == 0
        assert r["finite_missed"] == 0 and r["other_missed"] == 0
        assert r["finite_hits"] >= len(rays) / 4
        if name == "room":
            assert r["nodes_1"] < 0.2 * r["finite_hits"] * 400                 # a walk, not a sweep (far origins may sweep: not bounded)


@pytest.mark.parametrize("base,case", sc.all_cases() + [sc.EXCLUDED])
def test_the_sets_are_not_vacuous(pkg, scenes, oracle, base, case):
    """By the oracle alone: every set has a quarter of its rays hitting, the rim set has rays on both sides of the rim, and the limit set
    has rays that flip between occluded and not within the seven limits."""
    d = sc.case_data(pkg, scenes, oracle, base, case)
    for name in ("room", "far", "rim"):
        for ray_type in (qs.RAY_PRIMARY, qs.RAY_REFLECTION):
            hits = d[name, ray_type]
            assert np.all(np.abs((d[name][:, 3:].astype(np.float64) ** 2).sum(axis=1) - 1.0) < 2.0 ** -21)     # the filter path takes them
            assert int(hits["hit"].sum()) >= len(hits) / 4, (name, ray_type)
    outside_hit, off_target = sc.rim_census(d)
    print("%s %s rim: %d rays, on the target from outside %d, off the target %d" % (base, case, len(d["rim"]), outside_hit, off_target))
    assert off_target >= 50
    assert outside_hit >= 50
    occ = d["limit_occluded"].reshape(-1, 2, len(sc.LIMIT_STEPS))                # [ray, base of the limits: length / t, step]
    flips = occ.any(axis=2) & ~occ.all(axis=2)
    hist = sc.flip_histogram(d["limit_occluded"], d["limit_step"])
    print("%s %s limit: %d rays, flipping around the length %d, around t %d, first occluded limit (float32 steps from its base): %r" % (
        base, case, len(occ), int(flips[:, 0].sum()), int(flips[:, 1].sum()), hist))
    assert len(d["limit"]) <= 2048 and int(flips[:, 0].sum()) >= 100
    assert len(hist) > 1, "every ray flips at the same neighbour"
