"""What Tracer.kernels() (crt_describe_kernels) says on every launch path of tests/test_gpu_frame_path.py, at four points of a context's
life: after creation, after a depth-3 frame, after a GI frame (depth 1, one sample, one ray per pixel) and after a further depth-3
frame -- and on a scene without a candidate filter.  The strings are the ones recorded from the library before a frame's kernels were
chosen from one plan and named from the launch tables (tests/golden/kernel_names.json): bench.py names the roofline's kernel with
them and the tests branch on them, so they may not drift from what is launched."""
import json
import os

import pytest

import degenerate_sets as dg
from test_gpu_frame_path import DEPTH, PATHS, SIZES, small_scene, tracer_of

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_names.json")
POINTS = ["created", "depth-3 frame", "GI frame", "depth-3 frame again"]
NO_FILTER = "no filter: degenerate_sets needle"


def names_sequence(pkg, tracer):
    """the whole kernels() dictionary at the four POINTS"""
    rows = [tracer.kernels()]
    tracer.render(max_depth=DEPTH)
    rows.append(tracer.kernels())
    tracer.render(options=pkg.make_options(1, use_gi=True, gi_sample_size=1, rays_per_pixel=1))
    rows.append(tracer.kernels())
    tracer.render(max_depth=DEPTH)
    rows.append(tracer.kernels())
    return dict(zip(POINTS, rows))


def tracer_for(pkg, scenes, name):
    if name == NO_FILTER:
        return tracer_of(pkg, scenes, dg.scene_of(scenes, "needle")[0])
    return tracer_of(pkg, scenes, small_scene(scenes, *SIZES[0]), **dict(PATHS)[name])


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


@pytest.mark.parametrize("name", [p[0] for p in PATHS] + [NO_FILTER])
def test_kernel_names_are_the_recorded_ones(pkg, scenes, golden, name):
    got = names_sequence(pkg, tracer_for(pkg, scenes, name))
    print("names:", json.dumps(got))
    assert got == golden["names"][name]


def test_the_golden_file_tells_by_pixel_from_by_slot(golden):
    """(so that the comparison above cannot pass on a file that says nothing: a filter context's bulk shadow pass is by pixel after a
    depth-3 frame and by slot after a GI frame, and a context without a filter names neither)"""
    assert golden["scene"] == {"generator": "tests/test_gpu_frame_path.py: small_scene", "width": SIZES[0][0], "height": SIZES[0][1], "max_depth": DEPTH}
    assert sorted(golden["names"]) == sorted([p[0] for p in PATHS] + [NO_FILTER])
    rows = golden["names"]["defaults"]
    assert [rows[p]["shadow0"] for p in POINTS] == ["bvh_trace_shadow<0u, 0, true>", "bvh_trace_shadow<0u, 0, true>",
                                                    "bvh_trace_shadow<0u, 0, false>", "bvh_trace_shadow<0u, 0, true>"]
    assert all(rows[p]["filter"] != "" and not rows[p]["filter"].startswith("none") for p in POINTS)
    assert all(golden["names"][NO_FILTER][p]["filter"].startswith("none (") for p in POINTS)
    assert golden["names"]["mode=lanes"]["created"]["all"] == "render_lanes<false>"
