"""The GPU paths away from unit scale and away from the origin (tests/scale_sets.py; the CPU side is tests/test_scale_filter.py): frames,
crt_trace_rays, crt_occluded_rays, crt_shade_hits and crt_shoot_rays against the CPU oracle, every float bit for bit (NaN equals
NaN), for every case of the grid -- and, through the statistics, WHICH walk answered: with a filter the filter kernels (rerouted ==
the rays whose winner is at no finite distance, fallback_frames == 0), at S_lo, where the scene has none, the reference-order walk."""
import numpy as np
import pytest

import query_sets as qs
import scale_sets as sc
import shade_sets as ss
import shoot_sets as shs
from helpers import assert_same_floats, assert_same_hits, assert_shaded, blob_to_scene, load_golden

pytestmark = pytest.mark.gpu
CASES = sc.all_cases()
_TRACERS = {}


def setup(pkg, scenes, oracle, base, case):
    d = sc.case_data(pkg, scenes, oracle, base, case)
    if (base, case) not in _TRACERS:
        _TRACERS[base, case] = pkg.Tracer(pkg.Scene(json_text=scenes.to_json(d["scene"])))
    tracer = _TRACERS[base, case]
    note = tracer.kernels()["filter"]
    filtered = not note.startswith("none")
    assert filtered == (case != "lo"), note
    if not filtered:
        assert "margin" in note, note                     # why: a triangle without a usable margin (csrc/crt_bvh.cpp: triangle_margin)
    return d, tracer, filtered


@pytest.mark.parametrize("base,case", CASES + [sc.EXCLUDED])
def test_frames(pkg, scenes, oracle, base, case):
    """64x36 at depth 3, on the default path and with bvh = 0: both are the oracle's frame.  (s = 1e6 lies beyond the range the analysis
    of the walk's direction components covers; the library neither refuses it nor errs: it has a filter and renders the oracle's frame.)"""
    d, tracer, filtered = setup(pkg, scenes, oracle, base, case)
    want, _ = d["oracle"].render(3)
    got = tracer.render(max_depth=3).copy()
    st = tracer.stats()
    print("scale %s %s: filter %s, frame %dx%d fallback_frames %d kernel %.3f ms" % (base, case, "yes" if filtered else "no (%s)" % tracer.kernels()["filter"],
                                                                                   tracer.width, tracer.height, st.fallback_frames, st.kernel_ms))
    assert_same_floats(got, want, "%s %s frame" % (base, case))
    if filtered:
        assert st.fallback_frames == 0
    plain = pkg.Tracer(pkg.Scene(json_text=scenes.to_json(d["scene"])), tuning=pkg.make_tuning(bvh=0))
    assert_same_floats(plain.render(max_depth=3), want, "%s %s frame, bvh=0" % (base, case))
    if base == "hw11" and case in sc.FIXTURE_CASES:       # the real reference's frame of the same scene (tests/golden/scale_*.npz)
        g = load_golden("scale_" + case)
        t2 = pkg.Tracer(pkg.Scene(json_text=scenes.to_json(blob_to_scene(g["blob"]))))
        assert_same_floats(t2.render(max_depth=g["depth"]), g["rgb"], "fixture scale_" + case)
        if filtered:
            assert t2.stats().fallback_frames == 0


@pytest.mark.parametrize("base,case", CASES)
def test_trace_rays(pkg, scenes, oracle, base, case):
    d, tracer, filtered = setup(pkg, scenes, oracle, base, case)
    for name in ("room", "far", "rim"):
        for ray_type in (qs.RAY_PRIMARY, qs.RAY_REFLECTION):
            rays, want = d[name], d[name, ray_type]
            assert int(want["hit"].sum()) >= len(rays) / 4
            got = tracer.trace_rays(rays, ray_type)
            st = tracer.query_stats()
            expected = qs.non_finite_winners(want) if filtered else len(rays)      # (tests/test_gpu_query_rays.py: check_closest)
            print("scale %s %s %s type %d: filter %s, rays %d hits %d (oracle %d) rerouted %d (expected %d) kernel %.3f ms" % (
                base, case, name, ray_type, "yes" if filtered else "no", st.rays, st.hits, int(want["hit"].sum()), st.rerouted, expected, st.kernel_ms))
            what = "%s %s %s type %d" % (base, case, name, ray_type)
            assert_same_hits(got, want, what)
            assert (st.rays, st.hits) == (len(rays), int(want["hit"].sum())), what
            assert st.rerouted == expected, what


@pytest.mark.parametrize("base,case", CASES)
def test_occluded_rays(pkg, scenes, oracle, base, case):
    d, tracer, filtered = setup(pkg, scenes, oracle, base, case)
    o = d["oracle"]
    sets = [("limits", d["limit"], d["limit_dist"], d["limit_occluded"]),
            ("room within half an extent", d["room"], np.float32(0.5 * d["extent"]), None),
            ("far, no limit", d["far"], np.float32(np.inf), None)]
    wants = {}
    for what, rays, dist, want in sets:
        if want is None:
            want = qs.oracle_occluded(o, rays, dist)
        wants[what] = want
        got = tracer.occluded_rays(rays, dist)
        st = tracer.query_stats()
        print("scale %s %s occlusion, %s: rays %d occluded %d (oracle %d) rerouted %d kernel %.3f ms" % (base, case, what, st.rays, st.hits, int(want.sum()), st.rerouted, st.kernel_ms))
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s %s %s: %d rays differ, first %d" % (base, case, what, bad.size, bad[0])
        assert (st.rays, st.hits) == (len(rays), int(want.sum()))
        if not filtered:
            assert st.rerouted == len(rays)
        elif np.all(np.isfinite(dist)):
            assert st.rerouted == 0                       # (a limited query is never refuted: tests/test_gpu_query_rays.py)
    room = wants["room within half an extent"]
    assert len(room) / 4 <= int(room.sum()) < len(room)                        # neither all nor nothing
    assert int(wants["far, no limit"].sum()) >= len(d["far"]) / 4             # (from outside, without a limit, nearly every ray is occluded)


@pytest.mark.parametrize("case", ["hi", "s1e3", "offset"])
@pytest.mark.parametrize("base", list(sc.BASES))
def test_shade_hits_and_shoot_rays(pkg, scenes, oracle, base, case):
    """Shadow rays start at point + normal * 1e-4, which is absolute: a large step at S_hi, none at all at s = 1e3 (below the
    coordinates' rounding)."""
    d, tracer, filtered = setup(pkg, scenes, oracle, base, case)
    o, scene = d["oracle"], d["scene"]
    fixed = ss.is_fixed_point(d["room"])                  # (the oracle's shoot normalises its direction: tests/shade_sets.py)
    rays, hits = np.ascontiguousarray(d["room"][fixed]), np.ascontiguousarray(d["room", qs.RAY_REFLECTION][fixed])
    status = ss.expected_status(pkg, scene, hits)
    assert int((status == pkg.SHADE_DIFFUSE).sum()) >= len(rays) / 4
    rgb, got_status = tracer.shade_hits(hits)
    st = tracer.query_stats()
    print("scale %s %s shade_hits: filter %s, records %d diffuse %d rerouted %d kernel %.3f ms" % (base, case, "yes" if filtered else "no", st.rays, st.hits, st.rerouted, st.kernel_ms))
    assert_shaded(pkg, rgb, got_status, status, ss.oracle_colours(o, rays), "%s %s shade_hits" % (base, case))
    assert (st.rays, st.hits) == (len(hits), int((status == pkg.SHADE_DIFFUSE).sum()))
    shot = d["room"][:1024]
    got = tracer.shoot_rays(shot, qs.RAY_REFLECTION, max_depth=3)
    print("scale %s %s shoot_rays: rays %d" % (base, case, len(shot)))
    assert_same_floats(got, shs.oracle_colours(o, shot, 3), "%s %s shoot_rays" % (base, case))
