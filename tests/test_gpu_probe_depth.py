"""The probe volume's visibility term on the GPU (include/crt_hip.h: "Probe visibility"): crt_probe_depth_device and
crt_probe_irradiance_visible_device give the bits of the numpy restatement of csrc/probe_depth_rule.h (tests/probe_depth_sets.py;
tests/test_probe_depth_host.py holds that to the header), and crt_bake_probes_visible is crt_bake_probes with that depth pass: its depth
records are the projection of the hits the real reference gave for the rule's rays (tests/golden/probe_depth.npz), its SH records
crt_bake_probes' bytes.  Floats are compared bit for bit; two NaNs count as the same."""
import ctypes as C
import os

import numpy as np
import pytest

import degenerate_sets as ds
import probe_depth_sets as pd
import probe_sets as ps

pytestmark = pytest.mark.gpu
GUARD, SENT = 64, 0xA5
F32, U32 = np.float32, np.uint32


class Guarded:
    """a device array of n bytes, aligned to 64, between two runs of guard bytes (as in tests/test_gpu_probes.py)"""

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

    def fill(self):
        self.t[self.at:self.at + self.n] = SENT

    def intact(self):
        h = self.t.cpu().numpy()
        return bool(np.all(h[:self.at] == SENT) and np.all(h[self.at + self.n:] == SENT))

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "probe_depth.npz")
PLACE = dict(origin=(-1.25, 0.3, -4.0), spacing=(0.75, 1.3, 0.4), gi_seed=77)


@pytest.fixture(scope="module")
def world(pkg, scenes):
    """the HW11-like room, its tracer, the pinned volume and the recorded reference hits of its rays"""
    tracer = pkg.Tracer(pkg.Scene(json_text=scenes.to_json(ps.room(scenes))))
    v = ps.Volume(**ps.PIN_VOLUME)
    rays, _ = ps.rays_and_keys(v, 0, v.count)
    yield dict(tracer=tracer, volume=v, rays=rays, golden=np.load(GOLDEN))
    tracer.close()


def hit_records(pkg, hit, t):
    h = np.zeros(len(hit), dtype=pkg.HIT_DTYPE)
    h["hit"], h["t"] = hit, t
    h["normal"] = (0.0, 1.0, 0.0)
    return h


@pytest.mark.parametrize("R", ps.RAY_COUNTS)
def test_probe_depth_gives_the_rules_records(pkg, world, R):
    import torch
    tracer = world["tracer"]
    rng = np.random.default_rng(200 + R)
    for count in (1, 2, 65):                                      # 65: more probes than one workgroup's waves, and a last workgroup of one
        mx = 2.5 if count != 2 else 0.75
        v = ps.Volume(rays=R, nx=count, **PLACE)
        rays, _ = ps.rays_and_keys(v, 0, count)
        hit, t = pd.special_hits(rng, count * R, mx)
        hits = hit_records(pkg, hit, t)
        want = pd.project(rays, hit, t, count, R, mx)
        d_rays, d_hits = Guarded(torch, rays.nbytes, rays), Guarded(torch, hits.nbytes, hits)
        a, b = Guarded(torch, 512 * count), Guarded(torch, 512 * count)
        tracer.probe_depth_device(d_rays.ptr(), d_hits.ptr(), count, R, mx, a.ptr())
        tracer.probe_depth_device(d_rays.ptr(), d_hits.ptr(), count, R, mx, b.ptr())
        torch.cuda.synchronize()
        what = "R = %d, %d probes" % (R, count)
        pd.same_depth(a.values(F32), want, what)
        assert np.array_equal(a.values(np.uint8), b.values(np.uint8)), what + ": two runs differ"
        assert all(g.intact() for g in (d_rays, d_hits, a, b)), what + ": a guard byte was written"


def lookup_set(rng, dims, n):
    """a volume with random records and depth maps (for 3 x 2 x 4: a cell with eight and one with seven invalid corners), and n points: on
    probes, outside, inside, non-finite"""
    v = ps.Volume(rays=64, **dict(PLACE, **dims))
    rec = np.zeros(v.count, dtype=ps.PROBE_DTYPE)
    rec["coef"] = rng.uniform(-0.5, 2.0, (v.count, 9, 3)).astype(F32)
    rec["rays"] = 64
    rec["state"] = np.where((rng.uniform(size=v.count) < 0.25) & (np.arange(v.count) < 12), ps.INVALID, ps.VALID)
    if v.n == (3, 2, 4):
        rec["state"][[(iz * 2 + iy) * 3 + ix for iz in (0, 1) for iy in (0, 1) for ix in (0, 1)]] = ps.INVALID
        rec["state"][[(iz * 2 + iy) * 3 + 2 for iz in (0, 1) for iy in (0, 1)]] = [ps.VALID, ps.INVALID, ps.INVALID, ps.INVALID]
        rec["state"][-1] = 7
    mean = rng.uniform(0.05, 1.5, (v.count, 64)).astype(F32)
    depth = np.stack([mean, mean * mean + rng.uniform(0.0, 0.2, (v.count, 64)).astype(F32)], axis=2).astype(F32)
    span = v.spacing * (np.array(v.n) - 1)
    cells = np.array([v.origin + v.spacing * np.array([0.4, 0.3, 0.6]), v.origin + v.spacing * np.array([1.4, 0.3, 0.6])], dtype=F32)
    fixed = np.concatenate([ps.positions(v, np.arange(v.count)), cells, np.array([v.origin - 1.5, v.origin + span + 1.5], dtype=F32)]).astype(F32)
    if n < len(fixed):
        pts = fixed[rng.permutation(len(fixed))[:n]]
    else:
        pts = np.concatenate([fixed, (v.origin + rng.uniform(-0.2, 1.2, (n - len(fixed), 3)) * np.maximum(span, 1.0)).astype(F32)])
    nrm = rng.normal(size=pts.shape).astype(F32)
    if n >= 64:
        for k, value in enumerate([np.nan, np.inf, -np.inf]):
            pts[-1 - k, k] = value
            nrm[-4 - k, k] = value
    return v, rec, depth, pts, nrm


@pytest.mark.parametrize("n", [1, 64, 65, 1000])
def test_the_visible_lookup_gives_the_rules_colours(pkg, world, n):
    import torch
    tracer = world["tracer"]
    rng = np.random.default_rng(n)
    seen = set()
    for dims in (dict(nx=3, ny=2, nz=4), dict(nx=1, ny=1, nz=1)):
        v, rec, depth, pts, nrm = lookup_set(rng, dims, n if dims["nx"] == 3 or n < 1000 else 65)
        vis = pd.Visibility(v, normal_bias=0.0 if n == 64 else None)            # 0: a point AT a probe has dist == 0
        want_rgb, want_status = pd.lookup(v, vis, rec, depth, pts, nrm)
        d_rec, d_depth, d_pts, d_nrm = (Guarded(torch, a.nbytes, a) for a in (rec, depth, pts, nrm))
        d_rgb, d_status = Guarded(torch, 12 * len(pts)), Guarded(torch, len(pts))
        vol = pkg.make_probe_volume(**v.fields())
        p = pkg.make_probe_visibility(vol, **vis.fields())
        tracer.probe_irradiance_visible_device(vol, p, d_rec.ptr(), d_depth.ptr(), d_pts.ptr(), d_nrm.ptr(), len(pts), d_rgb.ptr(), d_status.ptr())
        torch.cuda.synchronize()
        what = "%r, %d points" % (dims, len(pts))
        ps.same_colours(d_rgb.values(F32).reshape(-1, 3), want_rgb, what)
        assert np.array_equal(d_status.values(np.uint8), want_status), what
        assert all(g.intact() for g in (d_rec, d_depth, d_pts, d_nrm, d_rgb, d_status)), what + ": a guard byte was written"
        # without a status array nothing is written for status
        d_rgb.fill()
        d_status.fill()
        tracer.probe_irradiance_visible_device(vol, p, d_rec.ptr(), d_depth.ptr(), d_pts.ptr(), d_nrm.ptr(), len(pts), d_rgb.ptr(), None)
        torch.cuda.synchronize()
        ps.same_colours(d_rgb.values(F32).reshape(-1, 3), want_rgb, what + ", no status")
        assert (d_status.values(np.uint8) == 0xA5).all() and d_status.intact()
        # the host variant
        rgb, status = tracer.probe_irradiance_visible(vol, p, rec, depth, pts, nrm)
        ps.same_colours(rgb, want_rgb, what + ", host variant")
        assert np.array_equal(status, want_status)
        seen |= set(want_status.tolist())
    if n == 1000:
        assert {0, 1, 8} <= seen, seen


def test_with_nothing_hidden_the_bytes_are_the_plain_lookups(pkg, world):
    import torch
    tracer = world["tracer"]
    rng = np.random.default_rng(31)
    v, rec, _, _, _ = lookup_set(rng, dict(nx=3, ny=2, nz=4), 1)
    vis = pd.Visibility(v)
    depth = np.tile(np.array([vis.max_distance, vis.max_distance * vis.max_distance], dtype=F32), (v.count, 64, 1))
    span = v.spacing * (np.array(v.n) - 1)
    pts = np.concatenate([(v.origin + rng.uniform(-0.05, 1.05, (300, 3)) * span).astype(F32), ps.positions(v, np.arange(v.count))])
    nrm = rng.normal(size=pts.shape).astype(F32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    d_rec, d_depth, d_pts, d_nrm = (Guarded(torch, a.nbytes, a) for a in (rec, depth, pts, nrm))
    plain, plain_status, got, got_status = Guarded(torch, 12 * len(pts)), Guarded(torch, len(pts)), Guarded(torch, 12 * len(pts)), Guarded(torch, len(pts))
    vol = pkg.make_probe_volume(**v.fields())
    tracer.probe_irradiance_device(vol, d_rec.ptr(), d_pts.ptr(), d_nrm.ptr(), len(pts), plain.ptr(), plain_status.ptr())
    tracer.probe_irradiance_visible_device(vol, pkg.make_probe_visibility(vol), d_rec.ptr(), d_depth.ptr(), d_pts.ptr(), d_nrm.ptr(), len(pts), got.ptr(),
                                           got_status.ptr())
    torch.cuda.synchronize()
    assert np.array_equal(got.values(np.uint8), plain.values(np.uint8)) and np.array_equal(got_status.values(np.uint8), plain_status.values(np.uint8))
    assert plain.values(F32).any() and len(set(plain_status.values(np.uint8).tolist())) >= 3


def test_bake_probes_visible_is_the_rule_around_the_references_hits(pkg, world):
    import torch
    tracer, v, z = world["tracer"], world["volume"], world["golden"]
    vol = pkg.make_probe_volume(**v.fields())
    vis = pd.Visibility(v)
    p = pkg.make_probe_visibility(vol)
    want = pd.project(world["rays"], z["pin_hit"], z["pin_t"], v.count, v.rays, vis.max_distance)
    plain = tracer.bake_probes(vol)
    rec, depth = tracer.bake_probes_visible(vol, p)
    assert rec.shape == depth.shape == (2, 2, 2)
    pd.same_depth(depth["moments"], want, "against tests/golden/probe_depth.npz")
    assert rec.tobytes() == plain.tobytes()
    st = tracer.probe_stats()
    assert (st.probes, st.invalid, st.rays) == (8, 0, 512) and st.total_ms > 0 and st.shoot_ms > 0 and st.project_ms > 0
    # the default visibility, three uneven chunks, and the records on the device as well
    tracer.set_probe_chunk(3)
    try:
        d_rec, d_depth = Guarded(torch, 128 * v.count), Guarded(torch, 512 * v.count)
        rec2, depth2 = tracer.bake_probes_visible(vol, d_probes_ptr=d_rec.ptr(), d_depth_ptr=d_depth.ptr())
        assert rec2.tobytes() == plain.tobytes() and depth2.tobytes() == depth.tobytes()
        assert d_rec.values(np.uint8).tobytes() == plain.tobytes() and d_depth.values(np.uint8).tobytes() == depth.tobytes()
        assert d_rec.intact() and d_depth.intact()
    finally:
        tracer.set_probe_chunk(0)
    # the plain bake gives the bytes it gave, after the visible one too
    assert tracer.bake_probes(vol).tobytes() == plain.tobytes()


def oracle_hit_t(o, rays):
    hit, t = np.zeros(len(rays), dtype=U32), np.zeros(len(rays), dtype=F32)
    for i, r in enumerate(rays):
        h, rec = o.trace(r[:3], r[3:], 2)
        hit[i], t[i] = h, rec[0] if h else 0
    return hit, t


def test_one_trace_serves_the_validity_and_the_depth_pass(pkg, scenes, oracle):
    """backface_limit 0.25 on the room with the closed box: states as crt_bake_probes gives them, depth as the rule"""
    scene = ps.box_room(scenes)
    tracer = pkg.Tracer(pkg.Scene(json_text=scenes.to_json(scene)))
    v = ps.Volume(**ps.BOX_VOLUME)
    vol = pkg.make_probe_volume(**v.fields())
    rays, _ = ps.rays_and_keys(v, 0, v.count)
    hit, t = oracle_hit_t(oracle.OracleScene(scenes.to_blob(scene)), rays)
    plain = tracer.bake_probes(vol)
    rec, depth = tracer.bake_probes_visible(vol)
    assert rec.tobytes() == plain.tobytes() and rec["state"].reshape(-1).tolist() == [ps.VALID, ps.INVALID, ps.VALID]
    pd.same_depth(depth["moments"], pd.project(rays, hit, t, v.count, v.rays, pd.Visibility(v).max_distance), "the closed box")
    assert tracer.probe_stats().invalid == 1
    tracer.close()


def test_a_scene_without_a_candidate_filter_bakes_the_rule(pkg, scenes, oracle):
    scene, _ = ds.scene_of(scenes, "needle")
    tracer = pkg.Tracer(pkg.Scene(json_text=scenes.to_json(scene)))
    assert tracer.kernels()["filter"].startswith("none")
    v = ps.Volume(**dict(ps.PIN_VOLUME, nz=1, backface_limit=0.5))
    vol = pkg.make_probe_volume(**v.fields())
    rays, _ = ps.rays_and_keys(v, 0, v.count)
    hit, t = oracle_hit_t(oracle.OracleScene(scenes.to_blob(scene)), rays)
    rec, depth = tracer.bake_probes_visible(vol)
    assert rec.tobytes() == tracer.bake_probes(vol).tobytes()
    pd.same_depth(depth["moments"], pd.project(rays, hit, t, v.count, v.rays, pd.Visibility(v).max_distance), "the needle scene")
    tracer.close()


def test_the_partition_scenes_lookup_is_the_restatements(pkg, scenes):
    z = np.load(GOLDEN)
    tracer = pkg.Tracer(pkg.Scene(json_text=scenes.to_json(pd.partition_room(scenes))))
    v = ps.Volume(**pd.PARTITION_VOLUME)
    vol = pkg.make_probe_volume(**v.fields())
    vis = pd.Visibility(v)
    p = pkg.make_probe_visibility(vol)
    rays, _ = ps.rays_and_keys(v, 0, v.count)
    rec, depth = tracer.bake_probes_visible(vol, p)
    ps.same_records(rec, ps.project(rays, z["part_rgb"], v.count, v.rays), "the partition scene's records")
    pd.same_depth(depth["moments"], pd.project(rays, z["part_hit"], z["part_t"], v.count, v.rays, vis.max_distance), "the partition scene's depth")
    for dark in (True, False):
        pts, nrm = pd.side_points(v, dark)
        want_rgb, want_status = pd.lookup(v, vis, rec, depth["moments"], pts, nrm)
        rgb, status = tracer.probe_irradiance_visible(vol, p, rec, depth, pts, nrm)
        ps.same_colours(rgb, want_rgb, "dark side" if dark else "lit side")
        assert np.array_equal(status, want_status)
        if dark:
            plain, _ = tracer.probe_irradiance(vol, rec, pts, nrm)
            assert (rgb < plain).all()
    tracer.close()


INVALID_VISIBILITY = [dict(size=0), dict(size=16), dict(size=24), dict(max_distance=0.0), dict(max_distance=-1.0), dict(max_distance=float("inf")),
                      dict(max_distance=float("nan")), dict(normal_bias=-1e-3), dict(normal_bias=float("inf")), dict(normal_bias=float("nan")),
                      dict(variance_floor=0.0), dict(variance_floor=-1.0), dict(variance_floor=float("inf")), dict(variance_floor=float("nan")),
                      dict(min_weight=0.0), dict(min_weight=-0.5), dict(min_weight=1.5), dict(min_weight=float("nan")), dict(min_weight=float("inf"))]
INVALID_VOLUMES = [dict(nx=0), dict(rays=0), dict(rays=4097), dict(nx=4096, ny=4096), dict(origin=(0, float("nan"), 0)), dict(spacing=(1, 0, 1)),
                   dict(backface_limit=1.5), dict(backface_limit=float("nan"))]


def test_invalid_calls_change_nothing(pkg, world):
    import torch
    tracer, L, v = world["tracer"], pkg.lib(), world["volume"]
    frame = tracer.render(max_depth=3)
    before = tracer.read_quantized().copy()
    stats_before = bytes(tracer.stats())
    o = pkg.make_options()
    good = pkg.make_probe_volume(**v.fields())
    vis = pkg.make_probe_visibility(good)
    out, out_depth = np.zeros(8, dtype=ps.PROBE_DTYPE), np.zeros(8, dtype=pd.DEPTH_DTYPE)
    dev = Guarded(torch, 4096)
    x = C.c_void_p(dev.ptr())

    def bake(vol=good, p=vis, options=o, d_probes=None, d_depth=None):
        return L.crt_bake_probes_visible(tracer.ctx, C.byref(vol) if vol is not None else None, C.byref(p) if p is not None else None,
                                         C.byref(options) if options is not None else None, out.ctypes.data, d_probes, out_depth.ctypes.data, d_depth)

    def lookup(vol=good, p=vis, probes=x, depth=x, points=x, normals=x, n=1, rgb=x):
        return L.crt_probe_irradiance_visible_device(tracer.ctx, C.byref(vol), C.byref(p) if p is not None else None, probes, depth, points, normals, n, rgb, x, None)

    for change in INVALID_VISIBILITY:
        bad = pkg.make_probe_visibility(good, **change)
        assert bake(p=bad) == pkg.CRT_ERR_INVALID, change
        assert lookup(p=bad) == pkg.CRT_ERR_INVALID, change
        assert L.crt_probe_irradiance_visible(tracer.ctx, C.byref(good), C.byref(bad), out.ctypes.data, out_depth.ctypes.data, out.ctypes.data, out.ctypes.data, 1,
                                              out.ctypes.data, None) == pkg.CRT_ERR_INVALID, change
    assert bake(p=None) == pkg.CRT_ERR_INVALID and lookup(p=None) == pkg.CRT_ERR_INVALID
    # crt_bake_probes' own refusals
    for change in INVALID_VOLUMES:
        bad = pkg.make_probe_volume(**dict(v.fields(), **change))
        assert bake(vol=bad) == pkg.CRT_ERR_INVALID, change
        assert lookup(vol=bad) == pkg.CRT_ERR_INVALID, change
    assert bake(vol=None) == pkg.CRT_ERR_INVALID and bake(options=None) == pkg.CRT_ERR_INVALID
    assert bake(d_probes=C.c_void_p(8)) == pkg.CRT_ERR_INVALID and bake(d_depth=C.c_void_p(8)) == pkg.CRT_ERR_INVALID
    for refused in (pkg.make_options(max_depth=64), pkg.make_options(use_gi=True, gi_sample_size=65), pkg.make_options(use_gi=True, max_depth=40, gi_sample_size=4)):
        assert bake(options=refused) == pkg.CRT_ERR_INVALID
    assert not out.view(np.uint8).any() and not out_depth.view(np.uint8).any()
    # the primitives: ranges, NULL arrays with work to do, alignment, max_distance
    depth = lambda rays=x, hits=x, count=1, R=64, mx=1.0, d=x: L.crt_probe_depth_device(tracer.ctx, rays, hits, count, R, mx, d, None)   # noqa: E731
    for kw in (dict(rays=None), dict(hits=None), dict(d=None), dict(d=C.c_void_p(dev.ptr() + 8)), dict(R=0), dict(R=4097), dict(count=1 << 24), dict(mx=0.0),
               dict(mx=-1.0), dict(mx=float("inf")), dict(mx=float("nan"))):
        assert depth(**kw) == pkg.CRT_ERR_INVALID, kw
    for kw in (dict(probes=None), dict(depth=None), dict(points=None), dict(normals=None), dict(rgb=None), dict(n=1 << 31),
               dict(depth=C.c_void_p(dev.ptr() + 8)), dict(probes=C.c_void_p(dev.ptr() + 8))):
        assert lookup(**kw) == pkg.CRT_ERR_INVALID, kw
    # nothing to do is CRT_OK and touches nothing
    assert depth(rays=None, hits=None, count=0, d=None) == pkg.CRT_OK
    assert lookup(probes=None, depth=None, points=None, normals=None, n=0, rgb=None) == pkg.CRT_OK
    assert L.crt_probe_irradiance_visible(tracer.ctx, C.byref(good), C.byref(vis), None, None, None, None, 0, None, None) == pkg.CRT_OK
    torch.cuda.synchronize()
    assert (dev.values(np.uint8) == 0xA5).all() and dev.intact()
    assert np.array_equal(tracer.read_quantized(), before) and bytes(tracer.stats()) == stats_before
    # a frame rendered before and after a visible bake is identical, and the bake leaves the colour buffer and the statistics alone
    tracer.bake_probes_visible(pkg.make_probe_volume(**dict(v.fields(), backface_limit=0.5)))
    assert np.array_equal(tracer.read_quantized(), before) and bytes(tracer.stats()) == stats_before
    again = tracer.render(max_depth=3)
    assert np.array_equal(again.view(np.uint32), frame.view(np.uint32))


def test_the_chain_in_a_stream_capture(pkg, world):
    """crt_probe_depth_device, then crt_probe_irradiance_visible_device, captured once on one stream and replayed twice: one chain, no
    parallel branch; both replays give the direct call's bytes"""
    import torch
    tracer, v, z = world["tracer"], world["volume"], world["golden"]
    vol = pkg.make_probe_volume(**v.fields())
    p = pkg.make_probe_visibility(vol)
    rng = np.random.default_rng(9)
    rec = np.zeros(v.count, dtype=ps.PROBE_DTYPE)
    rec["coef"] = rng.uniform(0.0, 2.0, (v.count, 9, 3)).astype(F32)
    rec["state"] = ps.VALID
    hits = hit_records(pkg, z["pin_hit"], z["pin_t"])
    span = v.spacing * (np.array(v.n) - 1)
    pts = (v.origin + rng.uniform(-0.1, 1.1, (200, 3)) * span).astype(F32)
    nrm = rng.normal(size=pts.shape).astype(F32)
    d_rays, d_hits, d_rec, d_pts, d_nrm = (Guarded(torch, a.nbytes, a) for a in (world["rays"], hits, rec, pts, nrm))
    depth, out, status = Guarded(torch, 512 * v.count), Guarded(torch, 12 * len(pts)), Guarded(torch, len(pts))
    mx = float(p.max_distance)

    def chain(stream=None):
        tracer.probe_depth_device(d_rays.ptr(), d_hits.ptr(), v.count, v.rays, mx, depth.ptr(), stream)
        tracer.probe_irradiance_visible_device(vol, p, d_rec.ptr(), depth.ptr(), d_pts.ptr(), d_nrm.ptr(), len(pts), out.ptr(), status.ptr(), stream)

    chain()
    torch.cuda.synchronize()
    direct = [g.values(np.uint8).copy() for g in (depth, out, status)]
    want_depth = pd.project(world["rays"], z["pin_hit"], z["pin_t"], v.count, v.rays, mx)
    pd.same_depth(depth.values(F32), want_depth, "the direct call's depth")
    want_rgb, want_status = pd.lookup(v, pd.Visibility(v), rec, want_depth, pts, nrm)
    ps.same_colours(out.values(F32).reshape(-1, 3), want_rgb, "the direct call's lookup")
    assert np.array_equal(status.values(np.uint8), want_status)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for _ in range(2):
        for g in (depth, out, status):
            g.fill()
        graph.replay()
        torch.cuda.synchronize()
        for g, want in zip((depth, out, status), direct):
            assert np.array_equal(g.values(np.uint8), want)
    assert all(g.intact() for g in (d_rays, d_hits, d_rec, d_pts, d_nrm, depth, out, status))
    del graph
