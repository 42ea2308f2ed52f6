"""Radiance queries in the GI mode (include/crt_hip.h: crt_shoot_rays_gi*), what needs no GPU: the declarations, the exports and the
bindings, the options' layout, and that the oracle's frames the GPU tests compare with (tests/shoot_gi_sets.py) are what
tests/test_gpu_shoot_rays_gi.py takes them for."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import shoot_gi_sets as gs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["crt_shoot_rays_gi", "crt_shoot_rays_gi_device"]


def header():
    return open(os.path.join(ROOT, "include", "crt_hip.h")).read()


def test_gi_symbols_are_declared_and_exported(pkg):
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    plain = C.CDLL(os.path.join(os.path.dirname(pkg.LIB_PATH), "libcrt_hip.so"))
    L = pkg.lib()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, text), name + " is not declared"
        assert name in pkg.DEVICE_SYMBOLS and hasattr(L, name) and hasattr(plain, name), name
    host = re.search(r"int crt_shoot_rays_gi\s*\((.*?)\);", text, flags=re.S).group(1)
    assert [re.sub(r"\s+", " ", a.strip()) for a in host.split(",")] == [
        "crt_ctx *ctx", "const crt_ray *rays", "const uint32_t *keys", "uint64_t n", "uint32_t ray_type", "const crt_options *options", "float *out_rgb"]
    device = re.search(r"int crt_shoot_rays_gi_device\s*\((.*?)\);", text, flags=re.S).group(1)
    assert [re.sub(r"\s+", " ", a.strip()) for a in device.split(",")] == [
        "crt_ctx *ctx", "const crt_ray *d_rays", "const uint32_t *d_keys", "uint64_t n", "uint32_t ray_type", "const crt_options *options", "float *d_rgb",
        "void *stream"]
    vp = C.c_void_p
    assert L.crt_shoot_rays_gi.argtypes == [vp, vp, vp, C.c_uint64, C.c_uint32, C.POINTER(pkg.Options), vp]
    assert L.crt_shoot_rays_gi_device.argtypes == [vp, vp, vp, C.c_uint64, C.c_uint32, C.POINTER(pkg.Options), vp, vp]
    # where the header said "not offered", it now points at the new calls
    contract = header()
    assert contract.count("crt_shoot_rays_gi*") >= 3 and "rays_per_pixel is NOT read" in contract


def test_python_wrappers_have_the_documented_signatures(pkg):
    sig = inspect.signature(pkg.Tracer.shoot_rays_gi)
    assert list(sig.parameters) == ["self", "rays", "keys", "ray_type", "options", "option_fields"]
    assert sig.parameters["keys"].default is None and sig.parameters["ray_type"].default == pkg.RAY_REFLECTION
    assert sig.parameters["options"].default is None and sig.parameters["option_fields"].kind == inspect.Parameter.VAR_KEYWORD
    dev = inspect.signature(pkg.Tracer.shoot_rays_gi_device)
    assert {"d_rays_ptr", "n", "d_rgb_ptr", "d_keys_ptr", "ray_type", "options", "stream_ptr"} <= set(dev.parameters)
    assert callable(pkg.Tracer.shoot_stats)
    # option fields by name make a GI options block
    o = pkg.Tracer._gi_options(None, dict(max_depth=3, gi_sample_size=4, gi_seed=11))
    assert (o.use_gi, o.max_depth, o.gi_sample_size, o.gi_seed) == (1, 3, 4, 11)


def test_options_layout(pkg):
    m = re.search(r"typedef struct crt_options \{(.*?)\} crt_options;", header(), flags=re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [re.sub(r"\s+", " ", f.strip()).split(" ")[1] for f in body.split(";") if f.strip()]
    assert fields == [n for n, _ in pkg.Options._fields_]
    offsets = {n: 4 * k for k, n in enumerate(fields)}   # ten 4-byte fields
    assert C.sizeof(pkg.Options) == 40
    assert (pkg.Options.gi_sample_size.offset, pkg.Options.monte_carlo_bias.offset, pkg.Options.gi_seed.offset) == (
        offsets["gi_sample_size"], offsets["monte_carlo_bias"], offsets["gi_seed"]) == (24, 32, 36)


def test_the_oracles_frames_are_not_empty_cases(scenes, oracle):
    """hw11 at 48x32, depth 3: with no samples the GI frame differs from the deterministic one in the glass sphere's shadow (the
    occlusion rule alone), with two samples it depends on the seed in most pixels; hw08 has no refractive mesh."""
    n = gs.W * gs.H
    plain = gs.plain_frame(scenes, oracle, "hw11", gs.DEPTH)
    rule = gs.differing_pixels(gs.gi_frame(scenes, oracle, "hw11", gs.DEPTH, 0), plain)
    seeds = gs.differing_pixels(gs.gi_frame(scenes, oracle, "hw11", gs.DEPTH, 2, 9), gs.gi_frame(scenes, oracle, "hw11", gs.DEPTH, 2, 10))
    samples = gs.differing_pixels(gs.gi_frame(scenes, oracle, "hw11", gs.DEPTH, 2, 9), plain)
    print("hw11: rule alone %d, seeds %d, samples %d of %d pixels" % (rule, seeds, samples, n))
    assert rule >= 100 and seeds > n // 2 and samples > n // 2
    assert gs.differing_pixels(gs.gi_frame(scenes, oracle, "hw11", gs.DEPTH, 0, 9), gs.gi_frame(scenes, oracle, "hw11", gs.DEPTH, 0, 10)) == 0
    assert gs.differing_pixels(gs.gi_frame(scenes, oracle, "hw08", gs.DEPTH, 0) + 0.0, gs.plain_frame(scenes, oracle, "hw08", gs.DEPTH) + 0.0) == 0
    assert np.array_equal(oracle.bucket_grid(gs.W, gs.H, 16), [[8 * (k // 4), 12 * (k % 4), 12, 8] for k in range(16)]), "the frames cover every pixel"
    for name in ("hw11", "hw08", "hw14"):
        frame = gs.gi_frame(scenes, oracle, name, gs.DEPTH, 2)
        assert not np.isnan(frame).any() and not np.any((frame == 0) & np.signbit(frame)), name
    # the other two cameras see the room, and the inside one the glass sphere's shadow
    for camera in gs.CAMERAS:
        frame = gs.gi_frame(scenes, oracle, "hw11", gs.DEPTH, 2, camera=camera)
        background = np.all(frame == np.float32([0.0, 0.5, 0.0]), axis=2).sum()
        print("hw11 %s: %d background pixels" % (camera, background))
        assert background < n // 2, camera


def test_pixel_keys_are_the_frames(scenes, oracle):
    keys = gs.pixel_keys(oracle, 9, 5)
    assert [int(k) for k in keys] == [oracle.gi_mix(oracle.gi_mix(9, p), 0) for p in range(5)]
    m = gs.look_at((0.0, 0.0, 0.0), (0.0, 0.0, -1.0))
    assert np.array_equal(m, np.eye(3, dtype=np.float32)), "looking down -z with y up is the identity camera"


def test_recorded_gi_times_are_complete():
    """profiles/shoot_rays_gi.json (tools/shoot_gi_time.py on an MI355X; no threshold is set for the ratio): the GI query on the camera's
    rays beside the GI frame of the same camera, options and seed, measured in the same session, with the rays per level."""
    import json
    doc = json.load(open(os.path.join(ROOT, "profiles", "shoot_rays_gi.json")))
    assert doc["repeats"] >= 20 and doc["warmup"] >= 5 and doc["max_depth"] == 3 and doc["gi_sample_size"] == 2
    assert doc["query_ms"] > 0 and doc["frame_ms"] > 0 and doc["query_equals_the_frame"] is True
    assert doc["rays"] == 960 * 540 == doc["level_rays"][0] and doc["levels"] == len(doc["level_rays"]) == 4
    assert all(b <= 2 * a for a, b in zip(doc["level_rays"], doc["level_rays"][1:])) and doc["rerouted"] >= 0
    assert doc["shadow_records"] > doc["rays"]
