"""The seams of a frame's launch path (csrc/crt_launch.hip: launch_frame): the ONE launch ahead of a frame's kernels
(csrc/kernel_stream.h: stream_frame_reset), which zeroes the counters and render_lanes' pixel counter, presets the shadow queue's fill
and -- where the level queue runs the frame -- the bulk shadow pass's split mark, and copies the frame's argument block from its pinned
ring slot to its device slot; and the one device-to-host copy behind the frame, which carries the counter block with the fallback total
in its last word.  What can go wrong there: a launch path that reads a stale or a neighbour's argument block (another camera, another
depth), a split mark that is not what the pass behind it must walk (the short last block of the shadow placement included), a ring
slot reused while its source is still being read, a fallback total that a frame's reset clears.  The frames are the smallest that have
each of these; every frame is compared with the oracle's bit for bit, and the statistics a sequence of frames leaves are the ones
recorded from the kernels before the launches were folded (tests/golden/frame_path_counts.json)."""
import importlib
import json
import math
import os

import numpy as np
import pytest

from helpers import assert_same_floats

pytestmark = pytest.mark.gpu

tiles = importlib.import_module("course-assignment-danielhalachev_amd.tiles")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_path_counts.json")
SC_COUNT, SC_SHADOW, SC_OVERFLOW = 0, 5 * 64, 5 * 64 + 2   # csrc/kernel_common.h: rays per level; shadow rays queued; the overflow word
SC_BVH_DIAG = 400                                         # csrc/kernel_bvh.h: the bounds-checked build's (flag, index) pairs
DEPTH = 3
SIZES = [(64, 48), (72, 40)]     # 48 tiles = three full blocks of the shadow placement; 45 tiles = 16 + 16 + 13: a short last block
PATHS = [("defaults", dict()),                                   # the level queue's launch WITH level 0, on a stream of its own
         ("level_queue=513", dict(level_queue=513)),             # ... behind level 0
         ("level_queue=4097", dict(level_queue=4097)),           # level 0 held back until the first launch has ended
         ("level_queue=0", dict(level_queue=0)),                 # level by level, bvh_trace_shadow<1> launched
         ("bvh=0", dict(bvh=0)),                                 # the plan kernels
         ("bvh=2", dict(bvh=2)),                                 # the bounds-checked build
         ("mode=lanes", dict(mode=1))]                           # render_lanes alone (MODE_LANES)


def small_scene(scenes, width, height):
    """A diffuse floor, a mirror sphere and a glass sphere under two lights: primary rays that end diffuse (fixed shadow slots), in a
    mirror (a chain of reflections whose diffuse ends queue shadow rays below level 0) and in glass (two children per hit); bucket
    size 8, so that the reference's buckets cover every pixel of both frame sizes."""
    materials = [{"type": "diffuse", "albedo": [0.75, 0.70, 0.55], "smooth_shading": False},
                 {"type": "reflective", "albedo": [0.90, 0.90, 0.92], "smooth_shading": True},
                 {"type": "refractive", "albedo": [0.0, 0.0, 0.0], "smooth_shading": True, "ior": 1.5}]
    objects = [scenes.quad(0, (-4.0, -1.0, 1.0), (4.0, -1.0, 1.0), (4.0, -1.0, -9.0), (-4.0, -1.0, -9.0), 2, 2),
               scenes.uv_sphere(1, (-1.0, -0.2, -4.2), 0.8, 10, 5),
               scenes.uv_sphere(2, (0.9, -0.3, -3.2), 0.7, 10, 5)]
    scene = {"settings": scenes._settings(width, height, bucket=8),
             "camera": dict(CAMERAS[0]),
             "lights": [{"intensity": 120, "position": [-2.0, 3.0, -1.0]}, {"intensity": 90, "position": [2.5, 2.0, -5.0]}],
             "materials": materials, "objects": objects}
    return scenes._strip_uvs(scene)


def yaw(angle):
    c, s = math.cos(angle), math.sin(angle)
    return [c, 0.0, -s, 0.0, 1.0, 0.0, s, 0.0, c]


CAMERAS = [{"position": [0.0, 0.3, 0.6], "matrix": [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]},
           {"position": [0.5, 0.7, 0.2], "matrix": yaw(0.12)}]


def walking_camera(k):
    """frame k's camera of the 70-frame run: every frame from a place of its own"""
    return {"position": [-0.7 + 0.02 * k, 0.3 + 0.003 * k, 0.6], "matrix": yaw(0.004 * k - 0.14)}


def tracer_of(pkg, scenes, scene, **tuning):
    return pkg.Tracer(pkg.Scene(json_text=scenes.to_json(scene)), tuning=pkg.make_tuning(**tuning) if tuning else None)


def violations(tracer):
    c = tracer.stream_counts()
    return [(k, int(c[SC_BVH_DIAG + 2 * k + 1])) for k in range(16) if c[SC_BVH_DIAG + 2 * k]]


def oracle_frame(oracle_scene, camera, depth):
    oracle_scene.set_camera(camera["position"], camera["matrix"])
    frame = oracle_scene.render(depth)[0].copy()
    frame.setflags(write=False)
    return frame


@pytest.fixture(scope="module")
def small(scenes, oracle):
    """size -> (scene, its oracle); (size, camera, depth) -> the oracle's frame, rendered once"""
    loaded, frames = {}, {}

    def scene_of(size):
        if size not in loaded:
            scene = small_scene(scenes, *size)
            loaded[size] = (scene, oracle.OracleScene(scenes.to_blob(scene)))
        return loaded[size]

    def want(size, cam, depth):
        key = (size, cam, depth)
        if key not in frames:
            frames[key] = oracle_frame(scene_of(size)[1], CAMERAS[cam], depth)
        return frames[key]
    return scene_of, want


def counts_of(tracer):
    """what the frame left in its counter block, of the words launch decisions are made from: rays per level, shadow rays, overflow"""
    c = tracer.stream_counts()
    return {"levels": [int(c[SC_COUNT + g]) for g in range(DEPTH + 1)], "shadow": int(c[SC_SHADOW]), "overflow": int(c[SC_OVERFLOW])}


def stats_of(tracer):
    st = tracer.stats()
    return {"fallback_frames": int(st.fallback_frames), "queue_regrows": int(st.queue_regrows)}


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name,tuning", PATHS, ids=[p[0] for p in PATHS])
def test_three_frames_on_every_launch_path(pkg, scenes, small, name, tuning, size):
    """The probing frame, the first queued frame and a settled frame of one context, on every launch path that reads the split mark or
    the argument block: each is the oracle's frame; no frame is redone by the last resort; the bounds-checked build records nothing."""
    scene, _ = small[0](size)
    want = small[1](size, 0, DEPTH)
    assert len(np.unique(want.reshape(-1, 3), axis=0)) > 50          # the spheres and their shadows are in the picture
    tracer = tracer_of(pkg, scenes, scene, **tuning)
    filtered = tracer.kernels().get("level0", "").startswith("bvh_trace_")
    assert filtered == (name not in ("bvh=0", "mode=lanes")), tracer.kernels()
    for frame in range(3):
        got = tracer.render(max_depth=DEPTH)
        assert_same_floats(got, want, "%s %dx%d frame %d" % ((name,) + size + (frame,)))
        assert tracer.stats().fallback_frames == 0
        if tuning.get("bvh") == 2:
            assert violations(tracer) == []
    if name != "mode=lanes":
        c = counts_of(tracer)
        fixed = (size[0] // 8) * (size[1] // 8) * 64 * 2     # level 0's fixed slots: two lights (its rays are not counted: one per pixel)
        assert c["levels"][1] > 0 and c["levels"][DEPTH] > 0 and c["overflow"] == 0
        assert c["shadow"] > fixed                           # ... and the deeper levels' shadow rays behind them


def render_packed(pkg, tracer, torch, depth, n_tiles):
    """one frame enqueued on the null stream into a buffer of its own; nothing waits for it"""
    packed = torch.zeros(n_tiles * 192, dtype=torch.float32, device=torch.device("cuda", 0))
    tracer.render_tiles_device(pkg.make_options(depth), 0, 1, packed.data_ptr())
    return packed


def test_options_change_between_frames_without_a_wait(pkg, scenes, small):
    """One context, camera and depth changing frame by frame, no synchronisation between the calls (a frame whose size and depth have
    just been rendered is enqueued and left): every frame is the oracle's frame for ITS camera and depth -- not its neighbour's, whose
    argument block lies one ring slot away."""
    import torch
    size = SIZES[0]
    scene, _ = small[0](size)
    tracer = tracer_of(pkg, scenes, scene)
    n_tiles = (size[0] // 8) * (size[1] // 8)
    sequence = [(0, 3), (1, 1), (0, 3), (1, 3), (0, 3), (1, 3), (0, 1), (1, 1), (0, 1), (1, 3)]
    outs = []
    for cam, depth in sequence:
        tracer.set_camera(CAMERAS[cam]["position"], CAMERAS[cam]["matrix"])
        outs.append(render_packed(pkg, tracer, torch, depth, n_tiles))
    torch.cuda.synchronize()
    assert not np.array_equal(small[1](size, 0, 3), small[1](size, 1, 3)) and not np.array_equal(small[1](size, 0, 3), small[1](size, 0, 1))
    for k, ((cam, depth), packed) in enumerate(zip(sequence, outs)):
        want = tiles.pack_tiles(small[1](size, cam, depth), 0, 1)
        assert_same_floats(packed.cpu().numpy().reshape(n_tiles, 64, 3), want, "frame %d (camera %d, depth %d)" % (k, cam, depth))
    tracer.synchronize()
    assert tracer.stats().fallback_frames == 0


def test_seventy_frames_reuse_the_ring_slots(pkg, scenes, oracle):
    """70 frames of 16x16 back to back on one context, each from a camera of its own: frames 64 .. 69 reuse the ring slots of frames
    0 .. 5 (events, pinned counters, pinned and device argument blocks)."""
    import torch
    scene = small_scene(scenes, 16, 16)
    o = oracle.OracleScene(scenes.to_blob(scene))
    tracer = tracer_of(pkg, scenes, scene)
    outs = []
    for k in range(70):
        cam = walking_camera(k)
        tracer.set_camera(cam["position"], cam["matrix"])
        outs.append(render_packed(pkg, tracer, torch, DEPTH, 4))
    torch.cuda.synchronize()
    wants = {k: oracle_frame(o, walking_camera(k), DEPTH) for k in (0, 63, 64, 69)}
    assert not np.array_equal(wants[0], wants[64]) and not np.array_equal(wants[63], wants[64])
    for k, want in wants.items():
        assert_same_floats(outs[k].cpu().numpy().reshape(4, 64, 3), tiles.pack_tiles(want, 0, 1), "frame %d of 70" % k)
    tracer.synchronize()
    assert tracer.stats().fallback_frames == 0


def statistics_sequence(pkg, scenes):
    """The sequence whose statistics tests/golden/frame_path_counts.json records: three frames on every launch path (64x48, depth 3),
    the counter block's words and crt_stats after each; then a context whose walks are given four stack entries (a test hook: its
    frames are redone by the last resort, one fallback each) and the built stack back -- the fallback total must survive every
    frame's reset and reach the host with the counter block."""
    out = {}
    scene = small_scene(scenes, *SIZES[0])
    for name, tuning in PATHS:
        tracer = tracer_of(pkg, scenes, scene, **tuning)
        rows = []
        for frame in range(3):
            tracer.render(max_depth=DEPTH)
            row = stats_of(tracer)
            if name != "mode=lanes":
                row.update(counts_of(tracer))
            rows.append(row)
        out[name] = rows
    tracer = tracer_of(pkg, scenes, scene)
    rows = []
    for stack in (4, 4, 0xFFFFFFFF, 0xFFFFFFFF):
        tracer.set_filter_stack(stack)
        tracer.render(max_depth=DEPTH)
        rows.append(stats_of(tracer))
    out["four stack entries, twice; the built stack, twice"] = rows
    return out


def test_statistics_are_the_ones_recorded_before_the_launches_were_folded(pkg, scenes, small):
    golden = json.load(open(GOLDEN))
    assert golden["scene"] == {"generator": "tests/test_gpu_frame_path.py: small_scene", "width": SIZES[0][0], "height": SIZES[0][1], "max_depth": DEPTH}
    got = statistics_sequence(pkg, scenes)
    print("statistics:", json.dumps(got))
    assert got == golden["statistics"]
    fallbacks = [r["fallback_frames"] for r in got["four stack entries, twice; the built stack, twice"]]
    # (the sequence does reach the last resort, and the total is kept once the frames fit again)
    assert fallbacks[0] >= 1 and fallbacks[1] > fallbacks[0] and fallbacks[2:] == [fallbacks[1]] * 2
