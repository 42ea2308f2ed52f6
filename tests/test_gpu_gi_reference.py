"""The GI mode on the GPU against the REAL reference, bit for bit: the fixtures tests/golden/gi_pairs_<scene>.npz (tests/gi_reference_sets.py)
hold the reference's shootRay colours and getRay rays under seeded engines, each with the key -- or the frame seed -- whose draws are
the same floats.  The query kernels (csrc/kernel_radiance.h: crt_shoot_rays_gi, _device, _enqueue), the sample-ray kernel
(crt_camera_sample_rays_device) and the frame kernels' GI builds (csrc/kernel_stream.h and the others, through render and
crt_render_progressive on every launch path) must give the reference's bits.  Nothing but tests/golden/ is read; NaN equals NaN.  One
Tracer per scene and tuning, made once."""
import ctypes as C

import numpy as np
import pytest

import gi_reference_sets as grs
import query_sets as qs
from helpers import assert_same_floats, blob_to_scene, same_bits
from test_gpu_frame_path import PATHS

pytestmark = pytest.mark.gpu
# the candidate filter on (the defaults; at these details only hw11 keeps one) and off (the reference-order walk for every ray): both
# are held to the same reference colours, so the hit cases give the same colours either way
VARIANTS = [("filter", dict()), ("bvh=0", dict(bvh=0))]
_tracers = {}


@pytest.fixture(scope="module")
def tracer_of(pkg, scenes, tmp_path_factory):
    def get(name, tag="filter", tuning=None):
        if (name, tag) not in _tracers:
            scene = blob_to_scene(grs.load_fixture(name)[0])
            folder = ""
            if scene.get("textures"):
                folder = str(tmp_path_factory.mktemp("gi_reference_bitmaps"))
                scenes.write_bitmaps(scene, folder)
            _tracers[(name, tag)] = pkg.Tracer(pkg.Scene(json_text=scenes.to_json(scene), folder=folder), tuning=pkg.make_tuning(**tuning) if tuning else None)
        return _tracers[(name, tag)]
    yield get
    for t in _tracers.values():
        t.close()
    _tracers.clear()


def gi_options(pkg, depth, seed=0):
    return pkg.make_options(depth, use_gi=True, gi_sample_size=grs.SAMPLES, rays_per_pixel=1, gi_seed=int(seed))


def families(fx):
    """(what, rays, keys, ray types, MAX_DEPTH, the reference's colours) of the query rays and of the rays below a mirror"""
    return [("first hit diffuse", fx["q_rays"], fx["hit_keys"][fx["q_pair"]], fx["q_type"], grs.Q_DEPTH, fx["q_rgb"]),
            ("below a mirror", fx["m_rays"], fx["m_keys"], fx["m_type"], grs.M_DEPTH, fx["m_rgb"])]


# ---- 1. the radiance queries
@pytest.mark.parametrize("tag,tuning", VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize("name", grs.SCENES)
def test_shoot_rays_gi_equal_the_reference(pkg, tracer_of, name, tag, tuning):
    import torch
    fx = grs.load_fixture(name)[1]
    tracer = tracer_of(name, tag, tuning)
    for what, rays, keys, types, depth, want in families(fx):
        assert len(rays) >= (grs.MIN_QUERY if depth == grs.Q_DEPTH else grs.MIN_MIRROR if name in grs.MIRROR_SCENES else 0)
        opt = gi_options(pkg, depth)
        for t in np.unique(types):
            sel = np.flatnonzero(types == t)
            r, k, w = np.ascontiguousarray(rays[sel]), np.ascontiguousarray(keys[sel]), want[sel]
            label = "%s %s %s type %d" % (name, tag, what, t)
            assert_same_floats(tracer.shoot_rays_gi(r, k, int(t), opt), w, label + ": crt_shoot_rays_gi")
            n = len(r)
            d_rays, d_keys = torch.from_numpy(r).cuda(), torch.from_numpy(k.view(np.int32)).cuda()
            d_rgb = torch.full((n + 1, 3), float("nan"), dtype=torch.float32, device="cuda")   # (one row more: must stay untouched)
            d_rep = torch.full((C.sizeof(pkg.ShootReport),), 0xEE, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            tracer.shoot_rays_gi_device(d_rays.data_ptr(), n, d_rgb.data_ptr(), d_keys.data_ptr(), int(t), opt)
            torch.cuda.synchronize()
            rgb = d_rgb.cpu().numpy()
            assert np.all(np.isnan(rgb[n:])), "written past the end"
            assert_same_floats(rgb[:n], w, label + ": crt_shoot_rays_gi_device")
            d_rgb.fill_(float("nan"))
            torch.cuda.synchronize()
            tracer.shoot_rays_gi_enqueue(d_rays.data_ptr(), n, d_rgb.data_ptr(), d_keys.data_ptr(), int(t), opt, d_report_ptr=d_rep.data_ptr())
            torch.cuda.synchronize()
            rep = pkg.ShootReport.from_buffer_copy(d_rep.cpu().numpy().tobytes())
            rgb = d_rgb.cpu().numpy()
            assert (rep.overflow, rep.dropped) == (0, 0) and np.all(np.isnan(rgb[n:]))
            assert_same_floats(rgb[:n], w, label + ": crt_shoot_rays_gi_enqueue")


def test_other_keys_give_other_colours(pkg, tracer_of):
    """the keys are read: the same rays with the keys K ^ 1 differ from the reference's colours in most cases"""
    fx = grs.load_fixture("hw11")[1]
    sel = np.flatnonzero(fx["q_type"] == qs.RAY_REFLECTION)
    got = tracer_of("hw11").shoot_rays_gi(np.ascontiguousarray(fx["q_rays"][sel]), fx["hit_keys"][fx["q_pair"][sel]] ^ np.uint32(1), qs.RAY_REFLECTION,
                                          gi_options(pkg, grs.Q_DEPTH))
    assert (got != fx["q_rgb"][sel]).any(axis=1).mean() >= 0.9


# ---- 2. the jittered camera rays
@pytest.mark.parametrize("name", grs.SCENES)
def test_camera_sample_rays_equal_the_references(tracer_of, name):
    """crt_camera_sample_rays_device(gi_seed, k, pixel list): the case's pixel in a list of three (its neighbours' rays are not the
    reference's: their keys are not matched), its ray the reference's getRay(row, col, true), its key the matched key."""
    import torch
    fx = grs.load_fixture(name)[1]
    tracer = tracer_of(name)
    n_pixels = tracer.width * tracer.height
    assert len(fx["j_rays"]) >= grs.MIN_JITTER
    d_rays = torch.zeros((4, 6), dtype=torch.float32, device="cuda")
    d_keys = torch.zeros((4,), dtype=torch.int32, device="cuda")
    got, keys = np.zeros((len(fx["j_rays"]), 6), dtype=np.float32), np.zeros(len(fx["j_rays"]), dtype=np.uint32)
    for i in range(len(fx["j_rays"])):
        pixel = int(fx["j_row"][i]) * tracer.width + int(fx["j_col"][i])
        at = i % 3
        listed = np.array([(pixel + 1 + j) % n_pixels for j in range(3)], dtype=np.int32)
        listed[at] = pixel
        d_pixels = torch.from_numpy(listed).cuda()
        d_rays.fill_(float("nan"))
        tracer.camera_sample_rays_device(int(fx["j_seed"][i]), int(fx["j_k"][i]), d_rays.data_ptr(), 3, d_keys.data_ptr(), d_pixels.data_ptr())
        torch.cuda.synchronize()
        rays = d_rays.cpu().numpy()
        assert np.all(np.isnan(rays[3:])), "written past the end"
        got[i], keys[i] = rays[at], d_keys.cpu().numpy().view(np.uint32)[at]
    assert np.array_equal(keys, fx["jitter_keys"][fx["j_pair"]])
    same_bits(got, fx["j_rays"], "%s: the reference's getRay(row, col, true)" % name)


# ---- 3. the frame kernels' GI builds
@pytest.mark.parametrize("path,tuning", PATHS, ids=[p[0] for p in PATHS])
@pytest.mark.parametrize("name", grs.SCENES)
def test_gi_frame_has_the_references_colour_at_the_pinned_pixel(pkg, tracer_of, name, path, tuning):
    """One small frame per pinned pixel, with the gi_seed that puts the matched key on that pixel's sample 0: the pixel is the reference's
    shootRay(getRay(row, col, false)) under the pair's seed, folded as renderRectangle folds one colour -- from render and from
    crt_render_progressive, on every launch path."""
    fx = grs.load_fixture(name)[1]
    tracer = tracer_of(name, "path " + path, tuning)
    assert len(fx["p_row"]) >= grs.MIN_PIXELS
    want = grs.frame_pixel(fx["p_rgb"])
    one_shot, progressive = np.zeros_like(want), np.zeros_like(want)
    for i in range(len(want)):
        opt = gi_options(pkg, grs.Q_DEPTH, fx["p_seed"][i])
        one_shot[i] = tracer.render(options=opt)[fx["p_row"][i], fx["p_col"][i]]
        progressive[i] = tracer.render_progressive(opt, 1)[fx["p_row"][i], fx["p_col"][i]]
    assert_same_floats(one_shot, want, "%s %s: render" % (name, path))
    assert_same_floats(progressive, want, "%s %s: crt_render_progressive" % (name, path))
    assert tracer.stats().fallback_frames == 0
