"""The temporal accumulation on the GPU (include/crt_hip.h: crt_temporal_device, crt_render_accumulated, crt_history_reset,
crt_history_frames): the kernel gives the bits of the documented rule (tests/temporal_sets.py restates it; tests/test_temporal_host.py holds
that to csrc/temporal_rule.h), the frame call is the rule chained over frames on the adaptive frame's state and the first hits of the
camera's rays, and nothing else of the frame moves.  Scenes and helpers: tests/shoot_gi_sets.py (48x32), tests/progressive_sets.py,
tests/adaptive_sets.py, tests/denoise_sets.py."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import adaptive_sets as ads
import denoise_sets as dns
import progressive_sets as ps
import temporal_sets as ts
from shoot_gi_sets import W, H, SEED, assert_same_values, case
from test_gpu_adaptive import settings as adaptive_settings, adaptive

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "course-assignment-danielhalachev_amd", "crt_animation")
PIXELS = W * H
GUARD = 64          # bytes before and after every output
SENT = 0xA5
FRAMES = [("hw11", 3, 2), ("hw12", 2, 0), ("hw14", 1, 1)]   # (scene, max_depth, gi_sample_size), as test_gpu_denoise.py's
# The camera's move of the frame tests: a pan about the world's y axis and a translation, through set_camera.  Condition, asserted by
# test_the_frame_is_the_rule from the restatement: at least half of the hit pixels keep a valid tap, at least one in twenty loses all.
PAN_DEGREES, SHIFT = 8.0, (0.25, 0.05, 0.1)


def make(pkg, setting):
    return pkg.make_temporal(max_history=setting[0], normal_min=setting[1], sigma_plane=setting[2])


@pytest.fixture
def hw11(pkg, scenes, oracle, tmp_path_factory):
    return case(pkg, scenes, oracle, "hw11", tmp_path_factory)


class Guarded:
    """a device array of n bytes, aligned to 64, between two runs of guard bytes"""

    def __init__(self, torch, values=None, n=None):
        raw = np.ascontiguousarray(values).view(np.uint8).reshape(-1) if values is not None else None
        self.n = len(raw) if raw is not None else n
        self.t = torch.full((self.n + 2 * GUARD + 64,), SENT, dtype=torch.uint8, device="cuda")
        self.at = (-self.t.data_ptr()) % 64 + GUARD
        if raw is not None and self.n:
            self.t[self.at:self.at + self.n] = torch.from_numpy(raw.copy()).cuda()

    def ptr(self):
        return self.t.data_ptr() + self.at

    def values(self, dtype):
        return np.frombuffer(self.t[self.at:self.at + self.n].cpu().numpy().tobytes(), dtype=dtype)

    def intact(self):
        h = self.t.cpu().numpy()
        return bool(np.all(h[:self.at] == SENT) and np.all(h[self.at + self.n:] == SENT))


def upload(torch, s):
    return dict(total=Guarded(torch, s["total"]), sq=Guarded(torch, s["sq"]), counts=Guarded(torch, s["counts"]), hits=Guarded(torch, s["hits"]))


def run_primitive(torch, pkg, tracer, setting, width, height, pose, prev, dev, with_var=True, with_valid=True, stream=None):
    """one crt_temporal_device call on guarded arrays; prev: a Guarded of records or None -> dict of Guarded outputs; nothing is waited for"""
    n = width * height
    out = dict(next=Guarded(torch, n=64 * n), rgb=Guarded(torch, n=12 * n), var=Guarded(torch, n=4 * n) if with_var else None,
               valid=Guarded(torch, n=n) if with_valid else None)
    tracer.temporal_device(make(pkg, setting), width, height, pkg.make_pose(*pose) if prev is not None else None, prev.ptr() if prev is not None else None,
                           dev["total"].ptr(), dev["sq"].ptr(), dev["counts"].ptr(), dev["hits"].ptr(), out["next"].ptr(), out["rgb"].ptr(),
                           d_out_var_ptr=out["var"].ptr() if with_var else None, d_out_valid_ptr=out["valid"].ptr() if with_valid else None,
                           stream_ptr=stream)
    return out


def check(out, want, what):
    ts.same_records(out["next"].values(ts.HISTORY_DTYPE), want[0], what)
    dns.same(out["rgb"].values(np.float32), want[1], what + ": colour")
    if out["var"] is not None:
        dns.same(out["var"].values(np.float32), want[2], what + ": variance")
    if out["valid"] is not None:
        dns.same(out["valid"].values(np.uint8), want[3], what + ": valid taps")
    assert all(g.intact() for g in out.values() if g is not None), what + ": a guard byte was written"


# ---- 1. the primitive against the restatement, bit for bit
@pytest.mark.parametrize("width,height", ts.SHAPES)
def test_the_primitive_is_the_rule(pkg, hw11, width, height):
    """on an hw11 context (48x32): the primitive's size is the caller's"""
    import torch
    tracer = hw11["tracer"]
    s = ts.synthetic(width, height)
    dev = upload(torch, s)
    prev = Guarded(torch, s["prev"])
    for setting in ts.SETTINGS:
        for with_prev in (True, False):
            want = ts.frame(setting, width, height, s["pose"] if with_prev else None, s["prev"] if with_prev else None, s["total"], s["sq"], s["counts"],
                            s["hits"])
            for with_var, with_valid in ((True, True), (False, False)) if setting == ts.DEFAULTS else ((True, True),):
                what = "%dx%d, %r, previous history %r, optional outputs %r" % (width, height, setting, with_prev, with_var)
                out = run_primitive(torch, pkg, tracer, setting, width, height, s["pose"], prev if with_prev else None, dev, with_var, with_valid)
                torch.cuda.synchronize()
                check(out, want, what)
    # the inputs are unchanged
    ts.same_records(prev.values(ts.HISTORY_DTYPE), s["prev"], "the previous history")
    dns.same(dev["total"].values(np.float32), s["total"], "sum")
    dns.same(dev["sq"].values(np.float32), s["sq"], "sq")
    assert np.array_equal(dev["counts"].values(np.uint32), s["counts"]) and dev["hits"].values(np.uint8).tobytes() == s["hits"].tobytes()
    assert prev.intact() and all(g.intact() for g in dev.values())


def test_two_calls_back_to_back_on_one_stream(pkg, hw11):
    """frame 2's d_prev is frame 1's d_next, with nothing waited for between them"""
    import torch
    tracer, (width, height) = hw11["tracer"], (37, 29)
    s = ts.synthetic(width, height)
    dev, prev = upload(torch, s), Guarded(torch, s["prev"])
    first = ts.frame(ts.DEFAULTS, width, height, s["pose"], s["prev"], s["total"], s["sq"], s["counts"], s["hits"])
    second = ts.frame(ts.DEFAULTS, width, height, s["pose"], first[0], s["total"], s["sq"], s["counts"], s["hits"])
    assert (second[3] != first[3]).any() and (second[1].view(np.uint32) != first[1].view(np.uint32)).any()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        a = run_primitive(torch, pkg, tracer, ts.DEFAULTS, width, height, s["pose"], prev, dev, stream=stream.cuda_stream)
        b = run_primitive(torch, pkg, tracer, ts.DEFAULTS, width, height, s["pose"], a["next"], dev, stream=stream.cuda_stream)
    stream.synchronize()
    check(a, first, "the first call")
    check(b, second, "the second call behind it")
    # ... and one at a time
    one = run_primitive(torch, pkg, tracer, ts.DEFAULTS, width, height, s["pose"], prev, dev)
    torch.cuda.synchronize()
    two = run_primitive(torch, pkg, tracer, ts.DEFAULTS, width, height, s["pose"], one["next"], dev)
    torch.cuda.synchronize()
    ts.same_records(b["next"].values(ts.HISTORY_DTYPE), two["next"].values(ts.HISTORY_DTYPE), "back to back against one at a time")
    dns.same(b["rgb"].values(np.float32), two["rgb"].values(np.float32), "back to back against one at a time: colour")


# ---- the restatement of a frame, fed by what is not under test
_colours = {}


def colours_of(pkg, tracer, name, depth, samples, seed, count, view):
    """colours float32 [count, PIXELS, 3]: sample s of every pixel for `seed` and the tracer's camera as it stands (`view` names it), from the
    merged primitives camera_sample_rays_device + shoot_rays_gi_device; made once"""
    import torch
    key = (name, depth, samples, seed, count, view)
    if key not in _colours:
        o = ps.frame_options(pkg, depth, samples, 1, seed=seed)
        rays = torch.zeros((PIXELS, 6), dtype=torch.float32, device="cuda")
        keys = torch.zeros((PIXELS,), dtype=torch.int32, device="cuda")
        rgb = torch.zeros((PIXELS, 3), dtype=torch.float32, device="cuda")
        out = np.zeros((count, PIXELS, 3), dtype=np.float32)
        for s in range(count):
            tracer.camera_sample_rays_device(seed, s, rays.data_ptr(), d_keys_ptr=keys.data_ptr())
            tracer.shoot_rays_gi_device(rays.data_ptr(), PIXELS, rgb.data_ptr(), d_keys_ptr=keys.data_ptr(), ray_type=pkg.RAY_PRIMARY, options=o)
            torch.cuda.synchronize()
            out[s] = rgb.cpu().numpy()
        out.setflags(write=False)
        _colours[key] = out
    return _colours[key]


def first_hits(pkg, tracer):
    """the hits of Tracer.trace_rays on the camera's rays as PRIMARY rays, for the tracer's camera as it stands"""
    import torch
    rays = torch.zeros((PIXELS, 6), dtype=torch.float32, device="cuda")
    tracer.camera_rays_device(rays.data_ptr())
    torch.cuda.synchronize()
    return tracer.trace_rays(rays.cpu().numpy(), pkg.RAY_PRIMARY)


def moved(camera):
    position, matrix = camera
    m = (np.asarray(matrix, dtype=np.float64).reshape(3, 3) @ ts.rotation(PAN_DEGREES, 0.0)).astype(np.float32).reshape(9)
    return (np.asarray(position, dtype=np.float32) + np.array(SHIFT, dtype=np.float32)).astype(np.float32), m


class Chain:
    """the restatement chained over frames: previous records and pose, as the context's two slots hold them"""

    def __init__(self, temporal=None):
        self.temporal, self.prev, self.pose = temporal or ts.DEFAULTS, None, None

    def frame(self, state, hits, pose, keep=True):
        out = ts.frame(self.temporal, W, H, self.pose, self.prev, state["total"], state["sq"], state["counts"], hits)
        if keep:
            self.prev, self.pose = out[0], pose
        return out


# ---- 2. the first frame is the denoiser's
def test_the_first_frame_is_the_denoisers(pkg, hw11):
    import torch
    tracer, a = hw11["tracer"], adaptive_settings(pkg)
    tracer.set_camera(*tracer.scene.camera())
    tracer.history_reset()
    assert tracer.history_frames() == 0
    adaptive(pkg, tracer, ps.frame_options(pkg, 3, 2, 1), a, 0, 5)
    state = ads.run(colours_of(pkg, tracer, "hw11", 3, 2, SEED, 8, "own"), a, 5)
    mean = torch.zeros((PIXELS, 3), dtype=torch.float32, device="cuda")
    var = torch.zeros((PIXELS,), dtype=torch.float32, device="cuda")
    for k in ("total", "sq"):
        state[k] = np.ascontiguousarray(state[k], dtype=np.float32)
    d = [torch.from_numpy(state["total"]).cuda(), torch.from_numpy(state["sq"]).cuda(), torch.from_numpy(state["counts"].view(np.int32)).cuda()]
    tracer.sample_variance_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), PIXELS, mean.data_ptr(), var.data_ptr())
    torch.cuda.synchronize()
    got, valid = tracer.render_accumulated(valid=True)
    dns.same(got, mean.cpu().numpy(), "no history, no filter: crt_sample_variance_device's mean of the frame's state")
    assert not valid.any() and tracer.history_frames() == 1
    tracer.history_reset()
    got, valid = tracer.render_accumulated(denoise=pkg.make_denoise(), valid=True)
    dns.same(got, tracer.render_denoised(), "no history, the default filter: crt_render_denoised")
    assert not valid.any() and tracer.history_frames() == 1


# ---- 3. the frame call is the rule, chained over frames
@pytest.mark.parametrize("name,depth,samples", FRAMES)
def test_the_frame_is_the_rule(pkg, scenes, oracle, name, depth, samples, tmp_path_factory):
    c = case(pkg, scenes, oracle, name, tmp_path_factory)
    tracer, a = c["tracer"], adaptive_settings(pkg)
    own = tracer.scene.camera()
    views = [("own", own), ("own", own), ("moved", moved(own))]
    tracer.history_reset()
    chain, d = Chain(), pkg.make_denoise()
    try:
        for f, (view, pose) in enumerate(views):
            tracer.set_camera(*pose)
            seed = SEED + f
            state = ads.run(colours_of(pkg, tracer, name, depth, samples, seed, 8, view), a)
            hits = first_hits(pkg, tracer)
            rgb, counts = tracer.render_adaptive(ps.frame_options(pkg, depth, samples, 1, seed=seed), a)
            assert np.array_equal(counts.reshape(PIXELS), state["counts"])
            records, colour, var, valid = chain.frame(state, hits, pose)
            got, got8, taps = tracer.render_accumulated(rgb8=True, valid=True)
            what = "%s, frame %d" % (name, f)
            dns.same(got, colour, what + ": crt_render_accumulated against the restatement chained")
            dns.same(taps, valid, what + ": valid taps")
            assert np.array_equal(got8, quantised(got)), what + ": out_rgb8 is the PPMColor quantisation of out_rgb"
            filtered = tracer.render_accumulated(denoise=d)
            dns.same(filtered, dns.denoise(colour, var, hits, H, W, d)[0], what + ": with the spatial filter")
            assert tracer.history_frames() == f + 1
            hit = hits["hit"] != 0
            kept, lost = int((hit & (valid > 0)).sum()), int((hit & (valid == 0)).sum())
            print(what, "hit pixels %d, with a valid tap %d, without %d" % (int(hit.sum()), kept, lost))
            if f == 0:
                assert kept == 0
            if f == 1:
                assert kept * 10 >= hit.sum() * 9, "a static camera keeps its history"
            if f == 2:   # the condition on the move
                assert kept * 2 >= hit.sum() and lost * 20 >= hit.sum(), (kept, lost, int(hit.sum()))
    finally:
        tracer.set_camera(*own)
        tracer.history_reset()


def quantised(rgb):
    """PPMColor's rule (Color.cpp:12-16), as crt_quantize_device states it"""
    c = np.asarray(rgb, dtype=np.float32)
    cl = np.where(c < 0, np.float32(0), np.where(c > 1, np.float32(1), c)).astype(np.float32)
    return (cl * np.float32(255)).astype(np.float32).astype(np.uint16).astype(np.uint8)


# ---- 4. idempotence and no double counting; 5. nothing else moves
def test_one_frame_is_merged_once_and_nothing_else_moves(pkg, hw11):
    tracer, a = hw11["tracer"], adaptive_settings(pkg)
    own = tracer.scene.camera()
    tracer.set_camera(*own)
    tracer.history_reset()
    try:
        o0, o1 = ps.frame_options(pkg, 3, 2, 1), ps.frame_options(pkg, 3, 2, 1, seed=SEED + 1)
        hits = first_hits(pkg, tracer)
        colours = [colours_of(pkg, tracer, "hw11", 3, 2, SEED + f, 8, "own") for f in range(2)]
        never = adaptive(pkg, tracer, o1, a, 0, 8)                       # frame 1, never accumulated
        chain = Chain()
        adaptive(pkg, tracer, o0, a, 0, 8)
        first = tracer.render_accumulated()
        dns.same(first, chain.frame(ads.run(colours[0], a), hits, own)[1], "frame 0")
        assert tracer.history_frames() == 1
        # frame 1: after pass 3, twice, and after pass 8: each merges frame 0's history with the frame as it stands
        adaptive(pkg, tracer, o1, a, 0, 3)
        before = (tracer.read_quantized(), tracer.progressive_samples(), tracer.progressive_active(), bytes(tracer.stats()))
        denoised_before = tracer.render_denoised()
        early = tracer.render_accumulated(valid=True)
        generation = tracer.query_scratch_generation()
        again = tracer.render_accumulated(valid=True)
        assert tracer.query_scratch_generation() == generation, "a second call allocates nothing"
        after = (tracer.read_quantized(), tracer.progressive_samples(), tracer.progressive_active(), bytes(tracer.stats()))
        assert np.array_equal(before[0], after[0]), "the persistent colour buffer"
        assert before[1:] == after[1:] and before[1] == 3, "progressive_samples, progressive_active, crt_get_stats"
        dns.same(tracer.render_denoised(), denoised_before, "crt_render_denoised before and after an accumulate call")
        dns.same(again[0], early[0], "two calls on an unchanged frame: colour")
        dns.same(again[1], early[1], "two calls on an unchanged frame: valid taps")
        dns.same(early[0], chain.frame(ads.run(colours[1], a, 3), hits, own, keep=False)[1], "previous + frame 1 after pass 3")
        assert tracer.history_frames() == 2
        rest = adaptive(pkg, tracer, o1, a, 3, 5)
        dns.same(rest[0], never[0], "the finished frame against the same frame never accumulated")
        assert np.array_equal(rest[1], never[1]), "its counts"
        late = tracer.render_accumulated()
        dns.same(late, chain.frame(ads.run(colours[1], a), hits, own)[1], "previous + the finished frame 1: frame 1 is not counted twice")
        assert tracer.history_frames() == 2, "crt_history_frames advances once a frame"
        # the history survives set_camera; history_reset makes the next frame a first frame again
        tracer.set_camera(*own)
        assert tracer.history_frames() == 2
        adaptive(pkg, tracer, o0, a, 0, 8)
        third = tracer.render_accumulated(valid=True)
        dns.same(third[0], chain.frame(ads.run(colours[0], a), hits, own)[1], "frame 2 merges frames 0 and 1")
        assert third[1].any() and tracer.history_frames() == 3
        tracer.history_reset()
        assert tracer.history_frames() == 0
        fresh = tracer.render_accumulated(valid=True)
        dns.same(fresh[0], first, "after crt_history_reset the frame is a first frame")
        assert not fresh[1].any() and tracer.history_frames() == 1
    finally:
        tracer.history_reset()


# ---- 6. refusals
def test_refusals(pkg, scenes, oracle, hw11):
    import torch
    tracer, L = hw11["tracer"], pkg.lib()
    o, a = ps.frame_options(pkg, 3, 2, 1), adaptive_settings(pkg)
    untouched, untouched8, taps = np.full((H, W, 3), 5.0, dtype=np.float32), np.full((H, W, 3), 5, dtype=np.uint8), np.full((H, W), 5, dtype=np.uint8)
    call = lambda t, d=None: L.crt_render_accumulated(tracer.ctx, C.byref(t) if t is not None else None, C.byref(d) if d is not None else None,
                                                      untouched.ctypes.data_as(C.c_void_p), untouched8.ctypes.data_as(C.c_void_p),
                                                      taps.ctypes.data_as(C.c_void_p))
    good = pkg.make_temporal()
    tracer.history_reset()
    # no frame under way
    tracer.set_camera(*tracer.scene.camera())
    assert call(good) == pkg.CRT_ERR_INVALID and b"no adaptive frame" in L.crt_last_error(tracer.ctx)
    tracer.render(options=ps.frame_options(pkg, 3, 2, 2))
    assert call(good) == pkg.CRT_ERR_INVALID and b"no adaptive frame" in L.crt_last_error(tracer.ctx)
    # a uniform progressive frame under way
    tracer.render_progressive(o, 2)
    assert call(good) == pkg.CRT_ERR_INVALID
    assert b"UNIFORM" in L.crt_last_error(tracer.ctx) and b"crt_render_adaptive with min_samples = max_samples" in L.crt_last_error(tracer.ctx)
    assert tracer.progressive_samples() == 2
    # a multi-device tracer
    both = pkg.Tracer(tracer.scene, devices=[0, 0])
    for f in (both.render_accumulated, both.history_reset, both.history_frames):
        with pytest.raises(RuntimeError):
            f()
    both.close()
    # each invalid field, in the middle of an adaptive frame
    adaptive(pkg, tracer, o, a, 0, 2)
    quantised_before = tracer.read_quantized()
    bad = [pkg.make_temporal(**f) for f in (dict(max_history=0.0), dict(max_history=-1.0), dict(max_history=float("nan")), dict(max_history=float("inf")),
                                            dict(normal_min=float("nan")), dict(normal_min=float("inf")), dict(normal_min=float("-inf")),
                                            dict(sigma_plane=-0.5), dict(sigma_plane=float("nan")), dict(sigma_plane=float("inf")))]
    wrong_size = pkg.make_temporal()
    wrong_size.size = 12
    for t in bad + [wrong_size, None]:
        assert call(t) == pkg.CRT_ERR_INVALID
    assert call(good, pkg.make_denoise(iterations=9)) == pkg.CRT_ERR_INVALID
    assert np.all(untouched == 5.0) and np.all(untouched8 == 5) and np.all(taps == 5)
    assert tracer.progressive_samples() == 2 and np.array_equal(tracer.read_quantized(), quantised_before) and tracer.history_frames() == 0
    # ... and the primitive's: nothing is enqueued
    n = 8 * 4
    buf = torch.full((64 * n + 16,), 3, dtype=torch.uint8, device="cuda")
    other = torch.full((64 * n + 16,), 3, dtype=torch.uint8, device="cuda")
    base, base2 = buf.data_ptr() + (-buf.data_ptr()) % 16, other.data_ptr() + (-other.data_ptr()) % 16
    pose = pkg.make_pose(*tracer.scene.camera())
    p = C.c_void_p
    prim = lambda t=good, w=8, h=4, pose=pose, prev=p(base2), total=p(base), sq=p(base), counts=p(base), hits=p(base), nxt=p(base), rgb=p(base): \
        L.crt_temporal_device(tracer.ctx, C.byref(t) if t is not None else None, w, h, C.byref(pose) if pose is not None else None, prev, total, sq, counts,
                              hits, nxt, rgb, None, None, None)
    for t in bad + [wrong_size, None]:
        assert prim(t=t) == pkg.CRT_ERR_INVALID
    for name in ("total", "sq", "counts", "hits", "nxt", "rgb"):
        assert prim(**{name: None}) == pkg.CRT_ERR_INVALID, name
    assert prim(pose=None) == pkg.CRT_ERR_INVALID                                            # a history without its pose
    assert prim(prev=p(base)) == pkg.CRT_ERR_INVALID and b"d_next must not be d_prev" in L.crt_last_error(tracer.ctx)
    assert prim(nxt=p(base + 4)) == pkg.CRT_ERR_INVALID and prim(prev=p(base2 + 8)) == pkg.CRT_ERR_INVALID
    assert prim(w=65536, h=32768) == pkg.CRT_ERR_INVALID and b"2^31" in L.crt_last_error(tracer.ctx)
    assert prim(w=0, h=4) == pkg.CRT_OK and prim(w=8, h=0) == pkg.CRT_OK
    torch.cuda.synchronize()
    assert torch.all(buf == 3).item() and torch.all(other == 3).item()
    # every refusal left the frame continuable
    rest = adaptive(pkg, tracer, o, a, 2, 6)
    want = ads.run(colours_of(pkg, tracer, "hw11", 3, 2, SEED, 8, "own"), a)
    assert np.array_equal(rest[1].reshape(PIXELS), want["counts"])
    assert_same_values(rest[0].reshape(PIXELS, 3), want["mean"], "the frame after the refused calls")


# ---- 7. it accumulates
# hw11 at 48x32, depth 3, 2 GI samples, min = max = 4 samples, a static camera, 4 frames with the seeds SEED .. SEED + 3; truth: the oracle's frame
# with rays_per_pixel = 64; RMSE over the hit pixels.  RATIO is the RMSE of the fourth frame, accumulated at crt_temporal_defaults and filtered at
# crt_denoise_defaults, over the RMSE of that frame's own unfiltered 4-sample mean, measured once on the GPU with the restatement fed from the
# merged primitives' colours (not the code under test); the session's numbers are below.  It must beat the spatial filter alone
# (test_gpu_denoise.RATIO); the library's frame is asserted with a 10 % margin, for nothing but the choice of truth.
# Measured: RMSE over the 1536 hit pixels: the fourth frame's own mean 0.04420, accumulated (16 samples' worth, unfiltered) 0.02383, accumulated
# and denoised 0.01971: ratio 0.4461, against 0.6304 for the spatial filter alone on one frame.
RATIO = 0.4461
SPATIAL_RATIO = 0.6304


def test_it_accumulates(pkg, scenes, oracle, hw11):
    tracer = hw11["tracer"]
    own = tracer.scene.camera()
    tracer.set_camera(*own)
    tracer.history_reset()
    a, d = adaptive_settings(pkg, 4, 4), pkg.make_denoise()
    truth = ps.oracle_frame(scenes, oracle, "hw11", 3, 2, 64)
    hits = first_hits(pkg, tracer)
    hit = hits["hit"] != 0
    chain = Chain()
    try:
        for f in range(4):
            state = ads.run(colours_of(pkg, tracer, "hw11", 3, 2, SEED + f, 8, "own")[:4], a)
            records, colour, var, valid = chain.frame(state, hits, own)
            rgb, counts = tracer.render_adaptive(ps.frame_options(pkg, 3, 2, 1, seed=SEED + f), a)
            assert np.all(counts == 4)
            got = tracer.render_accumulated(denoise=d)
        want = dns.denoise(colour, var, hits, H, W, d)[0]
        noisy, merged, clean = dns.rmse(state["mean"], truth, hit), dns.rmse(colour, truth, hit), dns.rmse(want, truth, hit)
        print("hw11, frame 4 of 4 x 4 samples: RMSE over %d hit pixels: the frame's mean %.5f, accumulated %.5f, accumulated and denoised %.5f, ratio %.4f"
              % (int(hit.sum()), noisy, merged, clean, clean / noisy))
        ratio = dns.rmse(got, truth, hit) / dns.rmse(rgb, truth, hit)
        print("the library's frame: ratio %.4f" % ratio)
        assert RATIO < SPATIAL_RATIO and ratio <= RATIO * 1.1
    finally:
        tracer.history_reset()


# ---- 8. the animation driver
def test_crt_animation_temporal(pkg, scenes, tmp_path):
    assert os.path.exists(EXE), "crt_animation is not built"
    scene = scenes.make("hw11", width=64, height=40, detail=0.2)
    scene["settings"]["image_settings"]["bucket_size"] = 16
    (tmp_path / "scene.crtscene").write_text(scenes.to_json(scene))
    orbit = ["--depth", "2", "--fps", "3", "--seconds", "1"]            # four frames
    gi = ["--gi", "2", "--seed", "41", "--adaptive", "0.1", "2", "4", "--denoise", "2"]
    lines = {}
    for tag, extra in (("plain", []), ("spatial", gi), ("temporal", gi + ["--temporal"])):
        r = subprocess.run([EXE, "scene.crtscene", tag + "_", *orbit, *extra], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr
        lines[tag] = json.loads(r.stdout.strip().splitlines()[-1])
        assert lines[tag]["frames"] == 4 and all((tmp_path / ("%s_%f.ppm" % (tag, k))).exists() for k in range(4))
    assert (tmp_path / "temporal_0.000000.ppm").read_bytes() == (tmp_path / "spatial_0.000000.ppm").read_bytes(), "frame 0 has no history yet"
    assert (tmp_path / "temporal_2.000000.ppm").read_bytes() != (tmp_path / "spatial_2.000000.ppm").read_bytes()
    assert lines["temporal"]["temporal"] is True and lines["spatial"]["temporal"] is False
    assert 0.0 < lines["temporal"]["valid_history_share"] <= 1.0 and lines["spatial"]["valid_history_share"] == 0.0
    # without --gi the driver is what it was
    assert sorted(lines["plain"]) == sorted(["frames", "width", "height", "depth", "frames_in_flight", "render_s", "frames_per_s", "with_ppm_s",
                                             "frames_per_s_with_ppm", "ppm_files"])
    for extra in (["--temporal"], ["--gi", "2", "--temporal"], ["--adaptive", "0.1", "2", "4"]):
        r = subprocess.run([EXE, "scene.crtscene", "no_", *orbit, *extra], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
        assert r.returncode != 0 and "usage:" in r.stderr and not (tmp_path / "no_0.000000.ppm").exists(), extra
