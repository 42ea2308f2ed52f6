"""Lightmap baking on the GPU (include/crt_hip.h: crt_bake_texels_device, crt_bake_dilate_device, crt_bake_lightmap, crt_get_bake_stats):
the primitives give the bits of the numpy restatement of csrc/bake_rule.h (tests/bake_sets.py; tests/test_bake_host.py holds that to the
header), and the frame-level call is that rule around the radiance queries: its covered texels are the colours the real reference gave for
the probe rays (tests/golden/bake_maps.npz) and the oracle's, its other texels the dilation's copies."""
import ctypes as C
import os

import numpy as np
import pytest

import bake_sets as bs
import degenerate_sets as ds

pytestmark = pytest.mark.gpu
GUARD, SENT = 64, 0xA5


def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bake_maps.npz"))


class Guarded:
    """a device array of n bytes, aligned to 64, between two runs of guard bytes"""

    def __init__(self, torch, n, values=None):
        self.n = n
        self.t = torch.full((n + 2 * GUARD + 64,), SENT, dtype=torch.uint8, device="cuda")
        self.at = (-self.t.data_ptr()) % 64 + GUARD
        if values is not None:
            self.t[self.at:self.at + n] = torch.from_numpy(np.ascontiguousarray(values).view(np.uint8).reshape(-1).copy()).cuda()

    def ptr(self):
        return self.t.data_ptr() + self.at

    def values(self, dtype):
        return np.frombuffer(self.t[self.at:self.at + self.n].cpu().numpy().tobytes(), dtype=dtype)

    def intact(self):
        h = self.t.cpu().numpy()
        return bool(np.all(h[:self.at] == SENT) and np.all(h[self.at + self.n:] == SENT))


@pytest.fixture(scope="module")
def world(pkg, scenes, oracle, tmp_path_factory):
    """the scene of tests/bake_sets.py: its tracer, its oracle, the cases' mesh data, and the restatement's answers per (case, map)"""
    scene = bs.make_scene(scenes)
    hs = bs.host_scene(pkg, scenes, scene, str(tmp_path_factory.mktemp("bake")))
    tracer = pkg.Tracer(hs)
    mds = {name: bs.MeshData(pkg, hs, mesh) for name, mesh in bs.CASES.items()}
    cache = {}

    def want(name, width, height):
        if (name, width, height) not in cache:
            cache[(name, width, height)] = bs.texels(mds[name], width, height, 1e-3)
        return cache[(name, width, height)]
    yield dict(scene=scene, tracer=tracer, oracle=oracle.OracleScene(scenes.to_blob(scene)), mds=mds, want=want)
    tracer.close()


def maps_of(name):
    return bs.MAPS + ([bs.LARGE_MAP] if name == "hand" else [])


def run_texels(torch, pkg, tracer, mesh, width, height):
    n = width * height
    out = dict(texels=Guarded(torch, 48 * n), rays=Guarded(torch, 24 * n), work=Guarded(torch, pkg.Tracer.bake_work_bytes(width, height)))
    tracer.bake_texels_device(pkg.make_bake(mesh=mesh, width=width, height=height), out["texels"].ptr(), out["rays"].ptr(), out["work"].ptr())
    return out


@pytest.mark.parametrize("name", list(bs.CASES))
def test_the_primitive_gives_the_rules_records(pkg, world, name):
    import torch
    tracer, md = world["tracer"], world["mds"][name]
    for width, height in maps_of(name):
        what = "%s %dx%d" % (name, width, height)
        rec, rays, status = world["want"](name, width, height)
        a = run_texels(torch, pkg, tracer, md.mesh, width, height)
        b = run_texels(torch, pkg, tracer, md.mesh, width, height)
        torch.cuda.synchronize()
        got = a["texels"].values(bs.TEXEL_DTYPE).reshape(height, width)
        bs.same_records(got, rec, what)
        assert np.array_equal(got["status"], status), what
        got_rays = a["rays"].values(np.float32).reshape(height, width, 6)
        covered = status == bs.COVERED
        assert np.array_equal(got_rays[covered].view(np.uint32), rays[covered].view(np.uint32)), what + ": probe rays"
        # an empty texel's ray is not written
        assert np.all(a["rays"].values(np.uint8).reshape(height, width, 24)[~covered] == SENT), what
        # order independence: two runs, identical bytes
        assert np.array_equal(a["texels"].values(np.uint8), b["texels"].values(np.uint8)) and np.array_equal(a["rays"].values(np.uint8), b["rays"].values(np.uint8)), what
        assert all(g.intact() for g in list(a.values()) + list(b.values())), what + ": a guard byte was written"


def test_the_dilation_primitive_copies(pkg, world):
    import torch
    tracer = world["tracer"]
    rng = np.random.default_rng(11)
    for name, (width, height) in (("sphere", bs.MAPS[0]), ("knot", bs.MAPS[1]), ("hand", bs.MAPS[2])):
        status = world["want"](name, width, height)[2]
        rgb = rng.uniform(0, 1, (height, width, 3)).astype(np.float32)
        rgb[status == bs.EMPTY] = 0
        for passes in (0, 1, 2, 3, 100000):   # (more passes than the map is wide or high: max(W, H) are run)
            d_rgb, d_status = Guarded(torch, rgb.nbytes, rgb), Guarded(torch, status.nbytes, status)
            work = Guarded(torch, pkg.Tracer.bake_work_bytes(width, height))
            tracer.bake_dilate_device(width, height, passes, d_rgb.ptr(), d_status.ptr(), work.ptr())
            torch.cuda.synchronize()
            want_rgb, want_status = bs.dilate(rgb, status, passes)
            what = "%s %dx%d, %d passes" % (name, width, height, passes)
            assert np.array_equal(d_rgb.values(np.uint32), want_rgb.view(np.uint32).ravel()), what
            assert np.array_equal(d_status.values(np.uint8), want_status.ravel()), what
            assert d_rgb.intact() and d_status.intact() and work.intact(), what
            if passes == 100000:
                assert not (want_status == bs.EMPTY).any()


def same_colours(got, want, what):
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), "%s: %d of %d floats differ" % (what, int((~same).sum()), same.size)


@pytest.mark.parametrize("name", list(bs.CASES))
def test_the_lightmap_is_the_references(pkg, oracle, world, name):
    """without GI: the covered texels are tests/golden/bake_maps.npz bit for bit, EMPTY texels 0, DILATED texels the restatement's copies,
    out_rgb8 the quantised map, probe_self the oracle's count"""
    tracer, md, o = world["tracer"], world["mds"][name], world["oracle"]
    z = golden()
    for width, height in bs.MAPS[:2]:
        key = "%s_%dx%d" % (name, width, height)
        rec, rays, status = world["want"](name, width, height)
        rgb, got_status, texels, q8 = tracer.bake_lightmap(md.mesh, width, height, check_probes=True, rgb8=True)
        bs.same_records(texels, rec, key)
        covered = status == bs.COVERED
        same_colours(rgb[covered], z[key + "_rgb"], key + ": covered texels")
        want_rgb, want_status = bs.lightmap(z[key + "_rgb"], status, 2)
        same_colours(rgb, want_rgb, key)
        assert np.array_equal(got_status, want_status), key
        assert np.all(rgb[want_status == bs.EMPTY].view(np.uint32) == 0), key
        assert np.array_equal(q8.astype(np.uint16), oracle.quantize(rgb)), key
        st = tracer.bake_stats()
        assert (st.texels, st.covered, st.dilated) == (width * height, int(covered.sum()), int((want_status == bs.DILATED).sum())), key
        assert st.probe_self == int(z[key + "_self"]), (key, st.probe_self)
        if (width, height) == bs.MAPS[0]:
            ids, prays, precs = bs.probe_rays(md, width, height)
            assert st.probe_self == bs.oracle_self_hits(o, md, prays, precs), key
        assert st.total_ms > 0 and st.raster_ms > 0
    # dilate = 0 leaves every EMPTY texel 0; without check_probes probe_self is 0
    width, height = bs.MAPS[0]
    status = world["want"](name, width, height)[2]
    rgb, got_status, _ = tracer.bake_lightmap(md.mesh, width, height, dilate=0)
    assert np.array_equal(got_status, status) and np.all(rgb[status == bs.EMPTY].view(np.uint32) == 0)
    assert tracer.bake_stats().probe_self == 0 and tracer.bake_stats().dilated == 0
    # more passes than the map is wide or high
    rgb, got_status, _ = tracer.bake_lightmap(md.mesh, width, height, dilate=0xFFFFFFFF)
    assert not (got_status == bs.EMPTY).any()


def test_the_larger_map_is_the_oracles(pkg, world):
    """64 x 64, where the quad's shared diagonals lie on texel centres: the oracle's shoot on the restatement's probe rays"""
    tracer, md, o = world["tracer"], world["mds"]["quad"], world["oracle"]
    width, height = bs.MAPS[2]
    ids, rays, rec = bs.probe_rays(md, width, height)
    rgb, status, texels = tracer.bake_lightmap(md.mesh, width, height)
    same_colours(rgb.reshape(-1, 3)[ids], bs.oracle_shoot(o, rays), "quad 64x64")
    # the large route of the rasteriser inside the frame-level call
    width, height = bs.LARGE_MAP
    md = world["mds"]["hand"]
    want = world["want"]("hand", width, height)
    rgb, status, texels = tracer.bake_lightmap(md.mesh, width, height, dilate=1)
    bs.same_records(texels, want[0], "hand 96x64")


@pytest.mark.parametrize("name", ["sphere", "hand"])
def test_the_gi_lightmap_is_the_fold_of_the_gi_queries(pkg, oracle, world, name):
    tracer, md, o = world["tracer"], world["mds"][name], world["oracle"]
    width, height = bs.MAPS[0]
    ids, rays, rec = bs.probe_rays(md, width, height)
    status = world["want"](name, width, height)[2]
    seed = 4242
    opts = pkg.make_options(max_depth=2, use_gi=True, gi_sample_size=2, gi_seed=seed)
    oo = oracle.make_options(max_depth=2, use_gi=1, gi_sample_size=2)
    singles_oracle = [o.shoot_gi(rays, bs.keys(seed, ids, s), 2, oo) for s in range(3)]
    singles_gpu = [tracer.shoot_rays_gi(rays, keys=bs.keys(seed, ids, s), ray_type=pkg.RAY_REFLECTION, options=opts) for s in range(3)]
    for samples in (1, 3):
        what = "%s, %d samples" % (name, samples)
        rgb, got_status, _ = tracer.bake_lightmap(md.mesh, width, height, options=opts, samples=samples, dilate=0)
        assert np.array_equal(got_status, status), what
        got = rgb.reshape(-1, 3)[ids]
        same_colours(got, bs.fold(singles_oracle[:samples]), what + ": the oracle's fold")
        same_colours(got, bs.fold(singles_gpu[:samples]), what + ": the fold of one-sample queries")
        assert np.all(rgb[status == bs.EMPTY].view(np.uint32) == 0), what


def test_invalid_calls_change_nothing(pkg, world):
    tracer, L = world["tracer"], pkg.lib()
    frame = tracer.render(max_depth=3)
    before = tracer.read_quantized().copy()
    stats_before = bytes(tracer.stats())
    n_meshes = len(world["scene"]["objects"])
    good = dict(mesh=bs.CASES["quad"], width=13, height=7, samples=1, dilate=2, check_probes=0, probe_offset=1e-3)
    o = pkg.make_options()
    bad = [dict(mesh=n_meshes), dict(width=0), dict(height=0), dict(samples=0), dict(width=1 << 16, height=1 << 15),
           dict(probe_offset=0.0), dict(probe_offset=-1e-3), dict(probe_offset=float("inf")), dict(probe_offset=float("nan"))]
    out = np.zeros((7, 13, 3), dtype=np.float32)
    for change in bad:
        b = pkg.make_bake(**dict(good, **change))
        assert L.crt_bake_lightmap(tracer.ctx, C.byref(b), C.byref(o), None, None, None, None) == pkg.CRT_ERR_INVALID, change
        assert L.crt_bake_texels_device(tracer.ctx, C.byref(b), C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), None) == pkg.CRT_ERR_INVALID, change
    b = pkg.make_bake(**good)
    assert L.crt_bake_lightmap(tracer.ctx, C.byref(b), None, out.ctypes.data, None, None, None) == pkg.CRT_ERR_INVALID          # NULL options
    assert L.crt_bake_lightmap(tracer.ctx, None, C.byref(o), out.ctypes.data, None, None, None) == pkg.CRT_ERR_INVALID
    for refused in (pkg.make_options(max_depth=64), pkg.make_options(use_gi=True, gi_sample_size=65), pkg.make_options(use_gi=True, max_depth=40, gi_sample_size=4)):
        assert L.crt_bake_lightmap(tracer.ctx, C.byref(b), C.byref(refused), out.ctypes.data, None, None, None) == pkg.CRT_ERR_INVALID
    assert not out.any()
    assert np.array_equal(tracer.read_quantized(), before) and bytes(tracer.stats()) == stats_before
    # a frame rendered before and after a bake is identical, and the bake leaves the colour buffer and the statistics alone
    tracer.bake_lightmap(bs.CASES["quad"], 33, 70, check_probes=True)
    assert np.array_equal(tracer.read_quantized(), before) and bytes(tracer.stats()) == stats_before
    again = tracer.render(max_depth=3)
    assert np.array_equal(again.view(np.uint32), frame.view(np.uint32))


def raw_context(pkg, hs, uvs):
    """crt_create on a host scene's description with vertex_uvs replaced: None, or a float32 array of the same size"""
    L = pkg.lib()
    d = hs.desc
    keep = d.vertex_uvs
    d.vertex_uvs = uvs.ctypes.data_as(C.POINTER(C.c_float)) if uvs is not None else None
    ctx = C.c_void_p()
    try:
        assert L.crt_create(C.byref(d), 0, C.byref(ctx)) == pkg.CRT_OK
    finally:
        d.vertex_uvs = keep
    return ctx


def test_a_scene_without_vertex_uvs_is_refused(pkg, scenes):
    """a context created from a description without vertex_uvs: CRT_ERR_INVALID, and a frame rendered before keeps its bytes"""
    L = pkg.lib()
    hs = pkg.Scene(json_text=scenes.to_json(scenes.make("hw07", width=32, height=24, detail=0.25)))
    ctx = raw_context(pkg, hs, None)
    o = pkg.make_options(max_depth=1)
    rect = pkg.Rect(0, 0, 32, 24)
    assert L.crt_render(ctx, C.byref(o), C.byref(rect), 1, None) == pkg.CRT_OK
    before, after = np.zeros((24, 32, 3), dtype=np.uint8), np.zeros((24, 32, 3), dtype=np.uint8)
    assert L.crt_read_quantized(ctx, before.ctypes.data) == pkg.CRT_OK and before.any()
    b = pkg.make_bake(width=8, height=8)
    out = np.zeros((8, 8, 3), dtype=np.float32)
    assert L.crt_bake_lightmap(ctx, C.byref(b), C.byref(o), out.ctypes.data, None, None, None) == pkg.CRT_ERR_INVALID
    assert b"vertex_uvs" in L.crt_last_error(ctx)
    assert L.crt_bake_texels_device(ctx, C.byref(b), C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), None) == pkg.CRT_ERR_INVALID
    assert L.crt_read_quantized(ctx, after.ctypes.data) == pkg.CRT_OK
    assert np.array_equal(after, before) and not out.any()
    L.crt_destroy(ctx)


def test_a_nan_uv_covers_nothing_on_the_device(pkg, world):
    """the hand-made mesh with a NaN where the scene file has an infinity (a .crtscene cannot carry one): a context from the description
    with that vertex_uvs array bakes the same records"""
    L = pkg.lib()
    md = world["mds"]["hand"]
    uvs = md.uvs.copy()
    where = np.argwhere(np.isinf(uvs))
    assert len(where) == 1
    uvs[tuple(where[0])] = np.nan
    uvs = np.ascontiguousarray(uvs.reshape(-1), dtype=np.float32)
    ctx = raw_context(pkg, world["tracer"].scene, uvs)
    o = pkg.make_options()
    for width, height in maps_of("hand"):
        rec = world["want"]("hand", width, height)[0]
        got = np.zeros((height, width), dtype=bs.TEXEL_DTYPE)
        b = pkg.make_bake(mesh=md.mesh, width=width, height=height, dilate=0)
        assert L.crt_bake_lightmap(ctx, C.byref(b), C.byref(o), None, None, None, got.ctypes.data) == pkg.CRT_OK, L.crt_last_error(ctx)
        bs.same_records(got, rec, "NaN UV, %dx%d" % (width, height))
        assert not (got["triangle"] == md.tris[3]).any() and not (got["triangle"] == md.tris[2]).any()
    L.crt_destroy(ctx)


def test_the_primitives_in_a_stream_capture(pkg, scenes, world, tmp_path):
    """inside a capture crt_bake_texels_device refuses what would read back, allocate or wait -- a mesh without its list, a pending frame --
    before it enqueues anything; with the list in place both primitives are captured and the replays give the rule's bytes"""
    import torch
    scene = world["scene"]
    tracer = pkg.Tracer(bs.host_scene(pkg, scenes, scene, str(tmp_path)))   # a context of its own: no mesh has its list yet
    md = world["mds"]["sphere"]
    width, height = bs.MAPS[1]
    n = width * height
    rec, rays, status = world["want"]("sphere", width, height)
    bake = pkg.make_bake(mesh=md.mesh, width=width, height=height)
    texels, d_rays = Guarded(torch, 48 * n), Guarded(torch, 24 * n)
    work = Guarded(torch, pkg.Tracer.bake_work_bytes(width, height))
    call = lambda stream: tracer.bake_texels_device(bake, texels.ptr(), d_rays.ptr(), work.ptr(), stream)

    def refused_in_a_capture(word):
        x = torch.zeros(8, device="cuda")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = x + 1
            with pytest.raises(pkg.CrtError) as e:
                call(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert e.value.code == pkg.CRT_ERR_INVALID and word in str(e.value) and "captured" in str(e.value), str(e.value)
        graph.replay()
        torch.cuda.synchronize()
        assert y.cpu().tolist() == [1.0] * 8 and np.all(texels.values(np.uint8) == SENT), "a refused call enqueues nothing"
        del graph

    refused_in_a_capture("triangle list")
    call(None)                                   # outside a capture: the list is made
    torch.cuda.synchronize()
    bs.same_records(texels.values(bs.TEXEL_DTYPE).reshape(height, width), rec, "before the capture")
    tracer.render_async(pkg.make_options(max_depth=2))
    texels.t[texels.at:texels.at + texels.n] = SENT
    refused_in_a_capture("pending")
    tracer.wait()
    # captured: the records, then two dilation passes on a map of the caller's
    rng = np.random.default_rng(4)
    rgb = rng.uniform(0, 1, (height, width, 3)).astype(np.float32)
    rgb[status == bs.EMPTY] = 0
    d_rgb, d_status = Guarded(torch, rgb.nbytes, rgb), Guarded(torch, status.nbytes, status)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stream = torch.cuda.current_stream().cuda_stream
        call(stream)
        tracer.bake_dilate_device(width, height, 2, d_rgb.ptr(), d_status.ptr(), work.ptr(), stream)
    torch.cuda.synchronize()
    want_rgb, want_status = bs.dilate(rgb, status, 2)
    for _ in range(2):
        texels.t[texels.at:texels.at + texels.n] = SENT
        d_rgb.t[d_rgb.at:d_rgb.at + d_rgb.n] = torch.from_numpy(rgb.view(np.uint8).reshape(-1).copy()).cuda()
        d_status.t[d_status.at:d_status.at + d_status.n] = torch.from_numpy(status.reshape(-1).copy()).cuda()
        graph.replay()
        torch.cuda.synchronize()
        bs.same_records(texels.values(bs.TEXEL_DTYPE).reshape(height, width), rec, "a replay")
        covered = status == bs.COVERED
        assert np.array_equal(d_rays.values(np.float32).reshape(height, width, 6)[covered].view(np.uint32), rays[covered].view(np.uint32))
        assert np.array_equal(d_rgb.values(np.uint32), want_rgb.view(np.uint32).ravel()) and np.array_equal(d_status.values(np.uint8), want_status.ravel())
    assert all(g.intact() for g in (texels, d_rays, work, d_rgb, d_status))
    del graph
    tracer.close()


def test_a_scene_without_a_candidate_filter_bakes_the_rule(pkg, scenes, oracle):
    """degenerate_sets' needle scene has no candidate filter: its floor, given the quad's UVs again, bakes to the restatement's records and
    the oracle's colours, as a scene with the filter does"""
    scene, _ = ds.scene_of(scenes, "needle")
    scene = dict(scene, objects=[dict(ob) for ob in scene["objects"]])
    floor = ds.floor_mesh(scene)
    assert len(scene["objects"][floor]["vertices"]) == 4
    scene["objects"][floor]["uvs"] = np.array([(0.1, 0.1, 0), (0.9, 0.1, 0), (0.1, 0.8, 0), (0.9, 0.8, 0)], dtype=np.float32)
    hs = pkg.Scene(json_text=scenes.to_json(scene))
    tracer = pkg.Tracer(hs)
    assert tracer.kernels()["filter"].startswith("none")
    md = bs.MeshData(pkg, hs, floor)
    width, height = 33, 9
    ids, rays, rec = bs.probe_rays(md, width, height)
    assert 0 < len(ids) < width * height
    rgb, status, texels = tracer.bake_lightmap(floor, width, height, check_probes=True)
    bs.same_records(texels, bs.texels(md, width, height, 1e-3)[0], "needle scene's floor")
    o = oracle.OracleScene(scenes.to_blob(scene))
    same_colours(rgb.reshape(-1, 3)[ids], bs.oracle_shoot(o, rays), "needle scene's floor")
    assert tracer.bake_stats().probe_self == bs.oracle_self_hits(o, md, rays, rec)
    tracer.close()
