"""Probe-lit radiance on the GPU (include/crt_hip.h: "Probe-lit radiance"): crt_probe_light_hits_device gives the bits of the numpy restatement
of csrc/probe_lit_rule.h (tests/probe_lit_sets.py; tests/test_probe_lit_host.py holds that to the header); crt_shoot_rays_lit* is the GI
radiance query with gi_sample_size = 0 and that primitive behind every level's lighting; crt_render_probe_lit is the query on the camera's
rays.  Floats are compared bit for bit where the same kernel made them, and as float values where a `+ 0` lies between."""
import numpy as np
import pytest

import probe_depth_sets as pd
import probe_lit_sets as pl
import probe_sets as ps
import query_sets as qs
import shoot_gi_sets as gs
import shoot_sets as sh
from helpers import same_bits
from test_gpu_probe_depth import Guarded

pytestmark = pytest.mark.gpu
F32, U32 = np.float32, np.uint32
N = gs.W * gs.H
# a volume over the HW11-like room: 3 x 3 x 3 probes, about a third of the room apart
ROOM_VOLUME = dict(origin=(-2.0, -0.9, -6.5), spacing=(2.0, 1.0, 2.0), nx=3, ny=3, nz=3, rays=64, gi_seed=3, backface_limit=1.0)


def run_primitive(pkg, tracer, v, vis, rec, depth, hits, status, S, rgb, counts=True):
    """the primitive on guarded arrays -> (rgb, lit, unlit); every guard must be intact"""
    import torch
    volume = pkg.make_probe_volume(**v.fields())
    visibility = pkg.make_probe_visibility(volume, **vis.fields()) if vis is not None else None
    n = len(status)
    d_rec, d_depth = Guarded(torch, rec.nbytes, rec), Guarded(torch, depth.nbytes, depth)
    d_hits, d_status, d_rgb = Guarded(torch, hits.nbytes, hits), Guarded(torch, n, status), Guarded(torch, 12 * n, np.ascontiguousarray(rgb, dtype=F32))
    d_counts = Guarded(torch, 16, np.zeros(2, dtype=np.uint64))
    tracer.probe_light_hits_device(volume, visibility, d_rec.ptr(), d_depth.ptr() if vis is not None else None, d_hits.ptr(), d_status.ptr(), n, S,
                                   d_rgb.ptr(), d_counts.ptr() if counts else None)
    torch.cuda.synchronize()
    assert all(g.intact() for g in (d_rec, d_depth, d_hits, d_status, d_rgb, d_counts)), "a guard byte was written"
    c = d_counts.values(np.uint64)
    return d_rgb.values(F32).reshape(n, 3).copy(), int(c[0]), int(c[1])


@pytest.fixture(scope="module")
def room(pkg, scenes, oracle, tmp_path_factory):
    """the HW11-like room (a mirror and a glass sphere), its camera rays, and a volume baked with the GI radiance query at depth 1"""
    import torch
    c = gs.case(pkg, scenes, oracle, "hw11", tmp_path_factory)
    tracer = c["tracer"]
    volume = pkg.make_probe_volume(**ROOM_VOLUME)
    visibility = pkg.make_probe_visibility(volume)
    rec, depth = tracer.bake_probes_visible(volume, visibility, gs.gi_options(pkg, 1, 2))
    d_rec = torch.from_numpy(rec.reshape(-1).view(np.uint8).copy()).cuda()
    d_depth = torch.from_numpy(depth.reshape(-1).view(np.uint8).copy()).cuda()
    moments = np.ascontiguousarray(depth["moments"].reshape(-1, 64, 2))       # the depth records as the restatement reads them
    return dict(c, volume=volume, visibility=visibility, rec=rec.reshape(-1), depth=moments, d_rec=d_rec, d_depth=d_depth,
                v=ps.Volume(**ROOM_VOLUME))


def lit_device(room, rays, options, visible=False, ray_type=qs.RAY_PRIMARY):
    import torch
    tracer, n = room["tracer"], len(rays)
    d_rays = torch.from_numpy(np.array(rays)).cuda()
    d_rgb = torch.full((n + 1, 3), float("nan"), dtype=torch.float32, device="cuda")
    tracer.shoot_rays_lit_device(d_rays.data_ptr(), n, d_rgb.data_ptr(), room["volume"], room["d_rec"].data_ptr(),
                                 room["visibility"] if visible else None, room["d_depth"].data_ptr() if visible else None, ray_type, options)
    torch.cuda.synchronize()
    rgb = d_rgb.cpu().numpy()
    assert np.all(np.isnan(rgb[n:])), "written past the end"
    return rgb[:n]


def gi_device(room, rays, options, ray_type=qs.RAY_PRIMARY):
    import torch
    n = len(rays)
    d_rays = torch.from_numpy(np.array(rays)).cuda()
    d_rgb = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    room["tracer"].shoot_rays_gi_device(d_rays.data_ptr(), n, d_rgb.data_ptr(), None, ray_type, options)
    torch.cuda.synchronize()
    return d_rgb.cpu().numpy()


# ---- 1. the primitive against the restatement's bits
@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_the_primitive_gives_the_rules_colours(pkg, room, n, visible):
    tracer = room["tracer"]
    rng = np.random.default_rng(300 + n + (7 if visible else 0))
    for dims in (dict(nx=2, ny=2, nz=2), dict(nx=1, ny=1, nz=1), dict(nx=3, ny=2, nz=4)):
        v, rec, depth = pl.random_volume(rng, dims)
        vis = pd.Visibility(v) if visible else None
        pts, nrm = pl.random_points(rng, v, n)
        hits = np.zeros(n, dtype=pkg.HIT_DTYPE)
        hits["point"], hits["normal"], hits["hit"] = pts, nrm, 1
        status = pl.mixed_status(rng, n)
        direct = ps.special_colours(rng, n)
        lb, _ = pl.lbar(v, vis, rec, depth, pts, nrm)                       # computed once for every S
        diffuse = status == pl.DIFFUSE
        _, wlit, wunlit = pl.light(v, vis, rec, depth, hits, status, 2, direct)   # (the counts do not depend on S)
        for S in pl.SAMPLES if n != 1000 else (2,):
            what = "%s, n = %d, S = %d, %s" % (v.n, n, S, "visible" if visible else "plain")
            got, lit, unlit = run_primitive(pkg, tracer, v, vis, rec, depth, hits, status, S, direct)
            want = direct.copy()
            want[diffuse] = pl.combine(direct[diffuse], lb[diffuse], S)
            ps.same_colours(got, want, what)
            assert np.array_equal(got[~diffuse].view(U32), direct[~diffuse].view(U32)), what + ": a record that is not diffuse changed"
            assert (lit, unlit) == (wlit, wunlit) and lit + unlit == int(diffuse.sum()), what
            if S == 2:
                again, _, _ = run_primitive(pkg, tracer, v, vis, rec, depth, hits, status, S, direct, counts=False)
                assert np.array_equal(again.view(U32), got.view(U32)), what + ": two runs differ"
        if v.n == (3, 2, 4) and n >= 63:
            assert unlit >= 1                                                 # the cell of eight invalid corners


# ---- 2. S = 0: the GI query with no samples, as float values, with the hook running at every level
@pytest.mark.parametrize("depth", [0, 1, 3])
@pytest.mark.parametrize("name", ["hw11", "hw14"])
def test_no_samples_is_the_gi_query_with_none(pkg, scenes, oracle, room, name, depth, tmp_path_factory):
    c = gs.case(pkg, scenes, oracle, name, tmp_path_factory)
    world = dict(room, tracer=c["tracer"])
    opt = gs.gi_options(pkg, depth, 0)
    want = gi_device(world, c["rays"], opt)
    shadow_records = c["tracer"].shoot_stats().shadow_records
    for visible in (False, True):
        got = lit_device(world, c["rays"], opt, visible)
        gs.assert_same_values(got, want, "%s depth %d" % (name, depth))
        st, ls = c["tracer"].shoot_stats(), c["tracer"].probe_lit_stats()
        assert st.shadow_records == shadow_records == ls.lit + ls.unlit and ls.lit > 0


# ---- 3. rays whose first hit is diffuse: the primitive on (trace_rays' hits, the S = 0 colours), bit for bit
@pytest.mark.parametrize("visible", [False, True])
def test_first_hit_diffuse_rays_are_the_primitive(pkg, room, visible):
    tracer, rays = room["tracer"], room["rays"]
    hits = tracer.trace_rays(sh.normalized_rays(rays), qs.RAY_PRIMARY)   # (the rays as the query walks them: normalised on entry)
    direct = gi_device(room, rays, gs.gi_options(pkg, 3, 0))
    _, status = tracer.shade_hits(hits)
    diffuse = status == pl.DIFFUSE
    assert 100 < diffuse.sum() < N and (status == pl.RECURSES).sum() > 10
    vis = pd.Visibility(room["v"], **{k: getattr(room["visibility"], k) for k in ("max_distance", "normal_bias", "variance_floor", "min_weight")}) if visible else None
    for S in (2, 7):
        got = lit_device(room, rays, gs.gi_options(pkg, 3, S), visible)
        want, _, _ = run_primitive(pkg, tracer, room["v"], vis, room["rec"], room["depth"], hits, status, S, direct)
        same_bits(got[diffuse], want[diffuse], "S = %d" % S)
        # ... and the restatement's bits
        lb, _ = pl.lbar(room["v"], vis, room["rec"], room["depth"], hits["point"][diffuse], hits["normal"][diffuse])
        ps.same_colours(got[diffuse], pl.combine(direct[diffuse], lb, S), "S = %d, the restatement" % S)
        assert (lb > 0).any() and not np.array_equal(got[diffuse], direct[diffuse])
        # mirrors and glass show probe-lit surfaces too: recursing pixels change with S
        recurses = status == pl.RECURSES
        assert np.any(got[recurses] != direct[recurses])


# ---- 4. max_depth = 0: recursing records take the background, diffuse ones are lit
@pytest.mark.parametrize("visible", [False, True])
def test_depth_zero(pkg, room, visible):
    tracer, rays = room["tracer"], room["rays"]
    hits = tracer.trace_rays(sh.normalized_rays(rays), qs.RAY_PRIMARY)   # (the rays as the query walks them: normalised on entry)
    _, status = tracer.shade_hits(hits)
    direct = gi_device(room, rays, gs.gi_options(pkg, 0, 0))
    got = lit_device(room, rays, gs.gi_options(pkg, 0, 2), visible)
    vis = pd.Visibility(room["v"]) if visible else None
    diffuse, other = status == pl.DIFFUSE, status != pl.DIFFUSE
    gs.assert_same_values(got[other], direct[other], "records that are not diffuse")
    lb, _ = pl.lbar(room["v"], vis, room["rec"], room["depth"], hits["point"][diffuse], hits["normal"][diffuse])
    ps.same_colours(got[diffuse], pl.combine(direct[diffuse], lb, 2), "diffuse records")
    # (a recursing record's children are the background: the GI query's own colours, compared above)


# ---- 4b. a chain: level 1 is lit with its own records and normals, and the up-sweep carries the colour through unchanged
@pytest.fixture(scope="module")
def mirror_room(pkg, scenes, oracle, tmp_path_factory):
    """the room with a mirror of albedo exactly (1, 1, 1) in front of its back wall, and a volume baked in it"""
    import copy
    import torch
    scene = copy.deepcopy(gs.scene_of(scenes, "hw11"))
    scene["materials"].append({"type": "reflective", "albedo": [1.0, 1.0, 1.0], "smooth_shading": False})
    wall = scenes.quad(len(scene["materials"]) - 1, (-3.0, -1.5, -7.5), (3.0, -1.5, -7.5), (3.0, 2.5, -7.5), (-3.0, 2.5, -7.5))   # faces +z
    wall.pop("uvs", None)
    scene["objects"].append(wall)
    tracer = pkg.Tracer(pkg.Scene(json_text=scenes.to_json(scene)))
    volume = pkg.make_probe_volume(**ROOM_VOLUME)
    visibility = pkg.make_probe_visibility(volume)
    rec, depth = tracer.bake_probes_visible(volume, visibility, gs.gi_options(pkg, 1, 2))
    d_rec = torch.from_numpy(rec.reshape(-1).view(np.uint8).copy()).cuda()
    d_depth = torch.from_numpy(depth.reshape(-1).view(np.uint8).copy()).cuda()
    yield dict(scene=scene, tracer=tracer, rays=gs.case(pkg, scenes, oracle, "hw11", tmp_path_factory)["rays"], volume=volume,
               visibility=visibility, rec=rec.reshape(-1), depth=np.ascontiguousarray(depth["moments"].reshape(-1, 64, 2)), d_rec=d_rec,
               d_depth=d_depth, v=ps.Volume(**ROOM_VOLUME), mirror=len(scene["objects"]) - 1)
    tracer.close()


@pytest.mark.parametrize("visible", [False, True])
def test_a_chain_through_the_mirror_is_lit_at_its_terminal_hit(pkg, mirror_room, visible):
    """rays whose first hit is the white mirror and whose chain guide (one bounce, not cut) names the diffuse surface behind it: the lit
    colour is 0 + 1 * (the level-1 record's lit colour), so it equals, as float values, the primitive applied to the TERMINAL record -- the
    guide's record as guide_rays returns it (the primitive reads its point and normal alone) -- with the ray's S = 0 GI colour as direct
    light.  The same with the record trace_rays gives for the guide's terminal ray: the guide's point and normal are that record's bits."""
    m = mirror_room
    tracer, rays = m["tracer"], m["rays"]
    walked = sh.normalized_rays(rays)                                         # the rays as the query walks them (a guide walks a ray as given)
    first = tracer.trace_rays(walked, qs.RAY_PRIMARY)
    guide, gstatus, last = tracer.guide_rays(walked, qs.RAY_PRIMARY, max_bounces=1)
    chain = (first["hit"] != 0) & (first["mesh"] == m["mirror"]) & ((gstatus & 0x3F) == 1) & ((gstatus & 0x80) == 0) & (guide["hit"] != 0)
    terminal = tracer.trace_rays(last[chain], qs.RAY_REFLECTION)
    _, tstatus = tracer.shade_hits(terminal)
    keep = np.flatnonzero(chain)[tstatus == pl.DIFFUSE]                       # the chain ends diffuse
    terminal = terminal[tstatus == pl.DIFFUSE]
    assert len(keep) > 20, len(keep)
    assert np.array_equal(guide["point"][keep].view(U32), terminal["point"].view(U32)) and np.array_equal(guide["normal"][keep].view(U32), terminal["normal"].view(U32))
    s0 = gi_device(m, rays, gs.gi_options(pkg, 3, 0))[keep]
    vis = pd.Visibility(m["v"]) if visible else None
    status = np.full(len(keep), pl.DIFFUSE, dtype=np.uint8)
    for S in (2, 7):
        got = lit_device(m, rays, gs.gi_options(pkg, 3, S), visible)[keep]
        for records, what in ((np.ascontiguousarray(guide[keep]), "the guide's record"), (terminal, "the terminal ray's record")):
            want, lit, unlit = run_primitive(pkg, tracer, m["v"], vis, m["rec"], m["depth"], records, status, S, s0)
            gs.assert_same_values(got, want, "S = %d, %s" % (S, what))
            assert lit == len(keep) and unlit == 0
        assert np.any(got != s0)                                              # the volume's light is in it
        # ... and the restatement's bits for the terminal point and normal, with S: not level 0's normal (the mirror's), not S = 0
        lb, _ = pl.lbar(m["v"], vis, m["rec"], m["depth"], terminal["point"], terminal["normal"])
        gs.assert_same_values(got, pl.combine(s0, lb, S), "S = %d, the restatement" % S)


# ---- 5. chunking: passes of 64 rays change no colour and no count
def test_passes_of_64_rays_change_nothing(pkg, room):
    tracer, rays = room["tracer"], room["rays"]
    opt = gs.gi_options(pkg, 3, 2)
    full = lit_device(room, rays, opt, True)
    counts = (tracer.probe_lit_stats().lit, tracer.probe_lit_stats().unlit)
    host = tracer.shoot_rays_lit(rays, room["volume"], room["rec"], room["visibility"], room["depth"], qs.RAY_PRIMARY, opt)
    same_bits(host, full, "the host variant")
    tracer.set_query_chunks(64, 128, 64)
    try:
        same_bits(lit_device(room, rays, opt, True), full, "in passes of 64")
        ls = tracer.probe_lit_stats()
        assert (ls.lit, ls.unlit) == counts
    finally:
        tracer.set_query_chunks(0, 0, 0)


# ---- 6. the frame call
def test_the_frame_is_the_query_on_the_cameras_rays(pkg, room):
    import torch
    tracer = room["tracer"]
    opt = gs.gi_options(pkg, 3, 2)
    for visible in (False, True):
        frame, q8 = tracer.render_probe_lit(room["volume"], room["d_rec"].data_ptr(), room["visibility"] if visible else None,
                                            room["d_depth"].data_ptr() if visible else None, opt, quantized=True)
        d_rays = torch.zeros((N, 6), dtype=torch.float32, device="cuda")
        tracer.camera_rays_device(d_rays.data_ptr())
        torch.cuda.synchronize()
        want = lit_device(room, d_rays.cpu().numpy(), opt, visible)
        same_bits(frame.reshape(N, 3), want, "the float frame")
        d_in, d_q = torch.from_numpy(frame.reshape(-1).copy()).cuda(), torch.zeros(3 * N, dtype=torch.uint8, device="cuda")
        tracer.quantize_device(d_in.data_ptr(), 3 * N, d_q.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(q8.reshape(-1), d_q.cpu().numpy()) and np.array_equal(tracer.read_quantized(), q8)


# ---- 7. the refusal table: nothing is enqueued, nothing changes
def test_the_refusals(pkg, scenes, room):
    import torch
    tracer, rays = room["tracer"], room["rays"]
    d_rays = torch.from_numpy(np.array(rays)).cuda()
    d_rgb = torch.full((N, 3), 7.0, dtype=torch.float32, device="cuda")
    good = gs.gi_options(pkg, 2, 2)

    def refused(word, volume=room["volume"], visibility=None, probes=room["d_rec"].data_ptr(), depth=None, options=good, stream=None):
        with pytest.raises(pkg.CrtError) as e:
            tracer.shoot_rays_lit_device(d_rays.data_ptr(), N, d_rgb.data_ptr(), volume, probes, visibility, depth, qs.RAY_PRIMARY, options, stream)
        assert e.value.code == pkg.CRT_ERR_INVALID and word in str(e.value), str(e.value)
        with pytest.raises(pkg.CrtError) as e:
            tracer.render_probe_lit(volume, probes, visibility, depth, options)
        assert e.value.code == pkg.CRT_ERR_INVALID and word in str(e.value), str(e.value)

    refused("use_gi", options=pkg.make_options(2))
    refused("gi_sample_size", options=gs.gi_options(pkg, 2, 65))
    refused("volume", volume=pkg.make_probe_volume(nx=0))
    refused("probes", probes=None)
    refused("depth", visibility=room["visibility"])                          # a visibility without depth records
    refused("visibility", visibility=pkg.make_probe_visibility(room["volume"], min_weight=0.0), depth=room["d_depth"].data_ptr())
    L = pkg.lib()
    import ctypes as C
    assert L.crt_shoot_rays_lit_device(tracer.ctx, C.c_void_p(d_rays.data_ptr()), N, 0, C.byref(good), None, None, C.c_void_p(room["d_rec"].data_ptr()),
                                       None, C.c_void_p(d_rgb.data_ptr()), None) == pkg.CRT_ERR_INVALID                # a NULL volume
    # the primitive: crt_probe_irradiance_visible_device's refusals
    hits = torch.zeros((4, 48), dtype=torch.uint8, device="cuda")
    status = torch.ones(4, dtype=torch.uint8, device="cuda")
    for kw, word in ((dict(volume=pkg.make_probe_volume(ny=0)), "volume"), (dict(visibility=room["visibility"]), "depth"), (dict(S=65), "gi_sample_size"),
                     (dict(probes=room["d_rec"].data_ptr() + 4), "aligned"), (dict(n=1 << 31), "2^31")):
        with pytest.raises(pkg.CrtError) as e:
            tracer.probe_light_hits_device(kw.get("volume", room["volume"]), kw.get("visibility"), kw.get("probes", room["d_rec"].data_ptr()), None,
                                           hits.data_ptr(), status.data_ptr(), kw.get("n", 4), kw.get("S", 2), d_rgb.data_ptr())
        assert e.value.code == pkg.CRT_ERR_INVALID and word in str(e.value), str(e.value)
    # inside a capture: refused while nothing is enqueued, and the capture stays valid
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    side = torch.zeros(8, device="cuda")
    with torch.cuda.stream(stream):
        graph.capture_begin()
        side.add_(1.0)
        with pytest.raises(pkg.CrtError) as e:
            tracer.shoot_rays_lit_device(d_rays.data_ptr(), N, d_rgb.data_ptr(), room["volume"], room["d_rec"].data_ptr(), None, None, qs.RAY_PRIMARY, good,
                                         stream.cuda_stream)
        graph.capture_end()
    assert e.value.code == pkg.CRT_ERR_INVALID and "captured" in str(e.value), str(e.value)
    graph.replay()
    torch.cuda.synchronize()
    assert np.all(d_rgb.cpu().numpy() == 7.0), "a refused call wrote a colour"
    # a multi-device tracer has none of the calls
    multi = pkg.Tracer(pkg.Scene(json_text=scenes.to_json(room["scene"])), devices=[0, 0])
    try:
        for call in (lambda: multi.shoot_rays_lit(rays, room["volume"], room["rec"]), lambda: multi.render_probe_lit(room["volume"], 0),
                     lambda: multi.probe_lit_stats(), lambda: multi.shoot_rays_lit_device(0, 0, 0, room["volume"], 0),
                     lambda: multi.probe_light_hits_device(room["volume"], None, 0, 0, 0, 0, 0, 2, 0)):
            with pytest.raises(RuntimeError, match="multi-device"):
                call()
    finally:
        multi.close()
