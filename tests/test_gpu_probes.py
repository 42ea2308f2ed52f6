"""The irradiance probe volume on the GPU (include/crt_hip.h: "Irradiance probes"): the four primitives give the bits of the numpy restatement
of csrc/probe_rule.h (tests/probe_sets.py; tests/test_probes_host.py holds that to the header), and crt_bake_probes is that rule around the
radiance queries: its records are the projection of the colours the real reference gave for the rule's rays
(tests/golden/probe_volume.npz), of Tracer.shoot_rays' and of the oracle's.  Coefficients are compared bit for bit; two NaNs count as the
same (the sign of a NaN an operation makes is the machine's)."""
import ctypes as C
import os

import numpy as np
import pytest

import degenerate_sets as ds
import probe_sets as ps

pytestmark = pytest.mark.gpu
GUARD, SENT = 64, 0xA5
F32, U32 = np.float32, np.uint32


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

    def fill(self):
        self.t[self.at:self.at + self.n] = SENT

    def intact(self):
        h = self.t.cpu().numpy()
        return bool(np.all(h[:self.at] == SENT) and np.all(h[self.at + self.n:] == SENT))


@pytest.fixture(scope="module")
def world(pkg, scenes, oracle):
    """the HW11-like room: its tracer, its oracle, the pinned volume, the recorded reference colours and the restatement's records of them"""
    scene = ps.room(scenes)
    tracer = pkg.Tracer(pkg.Scene(json_text=scenes.to_json(scene)))
    v = ps.Volume(**ps.PIN_VOLUME)
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "probe_volume.npz"))
    rays, _ = ps.rays_and_keys(v, 0, v.count)
    yield dict(scene=scene, tracer=tracer, oracle=oracle.OracleScene(scenes.to_blob(scene)), volume=v, rays=rays, golden=z["rgb"],
               records=ps.project(rays, z["rgb"], v.count, v.rays))
    tracer.close()


VOLUMES = [dict(nx=1, ny=1, nz=1), dict(nx=2, ny=3, nz=1), dict(nx=3, ny=2, nz=4)]
PLACE = dict(origin=(-1.25, 0.3, -4.0), spacing=(0.75, 1.3, 0.4), gi_seed=77)


@pytest.mark.parametrize("R", ps.RAY_COUNTS)
def test_probe_rays_are_the_rules(pkg, world, R):
    import torch
    tracer = world["tracer"]
    for dims in VOLUMES:
        v = ps.Volume(rays=R, **dict(PLACE, **dims))
        vol = pkg.make_probe_volume(**v.fields())
        for first, count in ((0, v.count), (v.count // 2, v.count - v.count // 2)):
            what = "R = %d, %r, first %d" % (R, dims, first)
            want_rays, want_keys = ps.rays_and_keys(v, first, count)
            rays, keys = Guarded(torch, 24 * count * R), Guarded(torch, 4 * count * R)
            tracer.probe_rays_device(vol, first, count, rays.ptr(), keys.ptr())
            torch.cuda.synchronize()
            assert np.array_equal(rays.values(U32), want_rays.view(U32).ravel()), what
            assert np.array_equal(keys.values(U32), want_keys), what
            assert rays.intact() and keys.intact(), what + ": a guard byte was written"
        # without keys nothing is written for them
        rays = Guarded(torch, 24 * v.count * R)
        tracer.probe_rays_device(vol, 0, v.count, rays.ptr(), None)
        torch.cuda.synchronize()
        assert np.array_equal(rays.values(U32), ps.rays_and_keys(v, 0, v.count)[0].view(U32).ravel()) and rays.intact()


@pytest.mark.parametrize("R", ps.RAY_COUNTS)
def test_probe_project_gives_the_rules_records(pkg, world, R):
    import torch
    tracer = world["tracer"]
    rng = np.random.default_rng(100 + R)
    for count in (1, 2, 65):                                      # 65: more probes than one workgroup's waves, and a last workgroup of one
        v = ps.Volume(rays=R, nx=count, **PLACE)
        rays, _ = ps.rays_and_keys(v, 0, count)
        rgb = ps.special_colours(rng, count * R)
        want = ps.project(rays, rgb, count, R)
        d_rays, d_rgb = Guarded(torch, rays.nbytes, rays), Guarded(torch, rgb.nbytes, rgb)
        a, b = Guarded(torch, 128 * count), Guarded(torch, 128 * count)
        tracer.probe_project_device(d_rays.ptr(), d_rgb.ptr(), count, R, a.ptr())
        tracer.probe_project_device(d_rays.ptr(), d_rgb.ptr(), count, R, b.ptr())
        torch.cuda.synchronize()
        what = "R = %d, %d probes" % (R, count)
        got = a.values(ps.PROBE_DTYPE)
        ps.same_records(got, want, what)
        assert (got["pad"] == 0).all() and (got["rays"] == R).all() and (got["state"] == ps.VALID).all(), what
        assert np.array_equal(a.values(np.uint8), b.values(np.uint8)), what + ": two runs differ"
        assert all(g.intact() for g in (d_rays, d_rgb, a, b)), what + ": a guard byte was written"


def test_probe_validity_at_the_boundary_counts(pkg, world):
    import torch
    tracer = world["tracer"]
    rng = np.random.default_rng(3)
    for R, limit in ((64, 0.25), (100, 0.25), (63, 0.5), (65, 0.0), (64, 1.0)):
        v = ps.Volume(rays=R, nx=7, **PLACE)
        rays, _ = ps.rays_and_keys(v, 0, 7)
        edge = int(np.floor(float(F32(limit) * F32(R))))
        counts = [max(edge - 1, 0), edge, min(edge + 1, R), 0, R, R // 2, 1]
        hits = np.zeros((7, R), dtype=pkg.HIT_DTYPE)
        hits["hit"] = 1
        for p, back in enumerate(counts):
            order = rng.permutation(R)
            d = rays.reshape(7, R, 6)[p, :, 3:]
            hits["normal"][p] = -d
            hits["normal"][p, order[:back]] = d[order[:back]]
            hits["hit"][p, order[back:back + (R - back) // 3]] = 0
        rec = ps.project(rays, np.ones((7 * R, 3), dtype=F32), 7, R)
        want = ps.validity(rec, rays, hits["hit"].reshape(-1) != 0, hits["normal"].reshape(-1, 3), R, limit)
        assert want["back"].tolist() == counts
        d_rays, d_hits, d_rec = Guarded(torch, rays.nbytes, rays), Guarded(torch, hits.nbytes, hits), Guarded(torch, rec.nbytes, rec)
        tracer.probe_validity_device(d_rays.ptr(), d_hits.ptr(), 7, R, limit, d_rec.ptr())
        torch.cuda.synchronize()
        ps.same_records(d_rec.values(ps.PROBE_DTYPE), want, "R = %d, limit %r" % (R, limit))
        assert d_rays.intact() and d_hits.intact() and d_rec.intact()


def test_the_closed_box_makes_its_probe_invalid(pkg, scenes, oracle):
    """end to end: crt_bake_probes with backface_limit 0.25 on the room with the closed box; counts and states are the oracle's trace's,
    the coefficients the projection of the oracle's colours"""
    scene = ps.box_room(scenes)
    tracer = pkg.Tracer(pkg.Scene(json_text=scenes.to_json(scene)))
    o = oracle.OracleScene(scenes.to_blob(scene))
    v = ps.Volume(**ps.BOX_VOLUME)
    rays, _ = ps.rays_and_keys(v, 0, v.count)
    hit, normals = ps.oracle_hits(o, rays)
    want = ps.validity(ps.project(rays, ps.oracle_shoot(o, rays), v.count, v.rays), rays, hit, normals, v.rays, v.backface_limit)
    assert want["state"].tolist() == [ps.VALID, ps.INVALID, ps.VALID]
    got = tracer.bake_probes(pkg.make_probe_volume(**v.fields()))
    ps.same_records(got, want, "the closed box")
    st = tracer.probe_stats()
    assert (st.probes, st.invalid, st.rays) == (3, 1, 3 * v.rays)
    # the lookup between the box's probe and its neighbour uses the neighbour alone
    rgb, status = tracer.probe_irradiance(pkg.make_probe_volume(**v.fields()), got, [(-0.7, 0.0, -3.0), (0.0, 0.0, -3.0)], [(0, 1, 0), (0, 1, 0)])
    assert status.tolist() == [1, 0] and rgb[0].any() and not rgb[1].any()
    tracer.close()


def test_bake_probes_is_the_projection_of_the_references_colours(pkg, world):
    import torch
    tracer, v = world["tracer"], world["volume"]
    vol = pkg.make_probe_volume(**v.fields())
    got = tracer.bake_probes(vol)
    assert got.shape == (2, 2, 2)
    ps.same_records(got, world["records"], "against tests/golden/probe_volume.npz")
    ps.same_records(got, ps.project(world["rays"], tracer.shoot_rays(world["rays"], ray_type=pkg.RAY_REFLECTION), v.count, v.rays), "against Tracer.shoot_rays")
    st = tracer.probe_stats()
    assert (st.probes, st.invalid, st.rays) == (8, 0, 512) and st.total_ms > 0 and st.shoot_ms > 0 and st.project_ms > 0
    # three uneven chunks, and the records on the device as well
    tracer.set_probe_chunk(3)
    try:
        d = Guarded(torch, 128 * v.count)
        again = tracer.bake_probes(vol, d_probes_ptr=d.ptr())
        ps.same_records(again, world["records"], "in chunks of 3, 3 and 2 probes")
        ps.same_records(d.values(ps.PROBE_DTYPE), world["records"], "the device's records")
        assert d.intact()
    finally:
        tracer.set_probe_chunk(0)


def test_bake_probes_in_the_gi_mode_is_the_projection_of_the_gi_queries(pkg, oracle, world):
    tracer, o = world["tracer"], world["oracle"]
    v = ps.Volume(**dict(ps.PIN_VOLUME, gi_seed=4242))
    rays, keys = ps.rays_and_keys(v, 0, v.count)
    opts = pkg.make_options(max_depth=1, use_gi=True, gi_sample_size=1, gi_seed=999)   # (options.gi_seed is not read: the volume's makes the keys)
    got = tracer.bake_probes(pkg.make_probe_volume(**v.fields()), options=opts)
    colours = tracer.shoot_rays_gi(rays, keys=keys, ray_type=pkg.RAY_REFLECTION, options=opts)
    ps.same_records(got, ps.project(rays, colours, v.count, v.rays), "against Tracer.shoot_rays_gi under the rule's keys")
    ps.same_colours(colours, o.shoot_gi(rays, keys, 2, oracle.make_options(max_depth=1, use_gi=1, gi_sample_size=1)), "the oracle's GI colours")
    other = tracer.bake_probes(pkg.make_probe_volume(**dict(v.fields(), gi_seed=4243)), options=opts)
    assert not np.array_equal(other["coef"], got["coef"]), "another seed, other draws"


def test_a_scene_without_a_candidate_filter_bakes_the_rule(pkg, scenes, oracle):
    scene, _ = ds.scene_of(scenes, "needle")
    tracer = pkg.Tracer(pkg.Scene(json_text=scenes.to_json(scene)))
    assert tracer.kernels()["filter"].startswith("none")
    v = ps.Volume(**dict(ps.PIN_VOLUME, nz=1, backface_limit=0.5))
    rays, _ = ps.rays_and_keys(v, 0, v.count)
    o = oracle.OracleScene(scenes.to_blob(scene))
    hit, normals = ps.oracle_hits(o, rays)
    want = ps.validity(ps.project(rays, ps.oracle_shoot(o, rays), v.count, v.rays), rays, hit, normals, v.rays, v.backface_limit)
    ps.same_records(tracer.bake_probes(pkg.make_probe_volume(**v.fields())), want, "the needle scene")
    tracer.close()


INVALID_VOLUMES = [dict(nx=0), dict(ny=0), dict(nz=0), dict(rays=0), dict(rays=4097), dict(nx=4096, ny=4096), dict(nx=1 << 12, ny=1 << 6, nz=1 << 6),
                   dict(origin=(0, float("nan"), 0)), dict(origin=(float("inf"), 0, 0)), dict(spacing=(1, 0, 1)), dict(spacing=(1, 1, -1)),
                   dict(spacing=(float("inf"), 1, 1)), dict(spacing=(1, float("nan"), 1)), dict(backface_limit=-0.1), dict(backface_limit=1.5),
                   dict(backface_limit=float("nan"))]


def test_invalid_calls_change_nothing(pkg, world):
    import torch
    tracer, L, v = world["tracer"], pkg.lib(), world["volume"]
    frame = tracer.render(max_depth=3)
    before = tracer.read_quantized().copy()
    stats_before = bytes(tracer.stats())
    o = pkg.make_options()
    out = np.zeros(8, dtype=ps.PROBE_DTYPE)
    x = C.c_void_p(64)
    for change in INVALID_VOLUMES:
        bad = pkg.make_probe_volume(**dict(v.fields(), **change))
        assert L.crt_bake_probes(tracer.ctx, C.byref(bad), C.byref(o), out.ctypes.data, None) == pkg.CRT_ERR_INVALID, change
        assert L.crt_probe_rays_device(tracer.ctx, C.byref(bad), 0, 1, x, None, None) == pkg.CRT_ERR_INVALID, change
        assert L.crt_probe_irradiance_device(tracer.ctx, C.byref(bad), x, x, x, 1, x, None, None) == pkg.CRT_ERR_INVALID, change
        assert L.crt_probe_irradiance(tracer.ctx, C.byref(bad), out.ctypes.data, out.ctypes.data, out.ctypes.data, 1, out.ctypes.data, None) == pkg.CRT_ERR_INVALID
    good = pkg.make_probe_volume(**v.fields())
    assert L.crt_bake_probes(tracer.ctx, C.byref(good), None, out.ctypes.data, None) == pkg.CRT_ERR_INVALID             # NULL options
    assert L.crt_bake_probes(tracer.ctx, None, C.byref(o), out.ctypes.data, None) == pkg.CRT_ERR_INVALID
    assert L.crt_bake_probes(tracer.ctx, C.byref(good), C.byref(o), None, C.c_void_p(8)) == pkg.CRT_ERR_INVALID         # alignment
    for refused in (pkg.make_options(max_depth=64), pkg.make_options(use_gi=True, gi_sample_size=65), pkg.make_options(use_gi=True, max_depth=40, gi_sample_size=4)):
        assert L.crt_bake_probes(tracer.ctx, C.byref(good), C.byref(refused), out.ctypes.data, None) == pkg.CRT_ERR_INVALID
    assert not out.view(np.uint8).any()
    # a range outside the volume, NULL arrays with work to do, counts and ray counts out of range, a limit out of range
    assert L.crt_probe_rays_device(tracer.ctx, C.byref(good), 7, 2, x, None, None) == pkg.CRT_ERR_INVALID
    assert L.crt_probe_rays_device(tracer.ctx, C.byref(good), 0, 1, None, None, None) == pkg.CRT_ERR_INVALID
    assert L.crt_probe_rays_device(tracer.ctx, C.byref(good), 0, 1, C.c_void_p(8), None, None) == pkg.CRT_ERR_INVALID
    assert L.crt_probe_project_device(tracer.ctx, None, x, 1, 64, x, None) == pkg.CRT_ERR_INVALID
    assert L.crt_probe_project_device(tracer.ctx, x, x, 1, 0, x, None) == pkg.CRT_ERR_INVALID
    assert L.crt_probe_project_device(tracer.ctx, x, x, 1, 4097, x, None) == pkg.CRT_ERR_INVALID
    assert L.crt_probe_project_device(tracer.ctx, x, x, 1 << 24, 64, x, None) == pkg.CRT_ERR_INVALID
    assert L.crt_probe_validity_device(tracer.ctx, x, None, 1, 64, 0.5, x, None) == pkg.CRT_ERR_INVALID
    assert L.crt_probe_validity_device(tracer.ctx, x, x, 1, 64, 1.5, x, None) == pkg.CRT_ERR_INVALID
    assert L.crt_probe_validity_device(tracer.ctx, x, x, 1, 64, float("nan"), x, None) == pkg.CRT_ERR_INVALID
    assert L.crt_probe_irradiance_device(tracer.ctx, C.byref(good), x, None, x, 1, x, None, None) == pkg.CRT_ERR_INVALID
    assert L.crt_probe_irradiance_device(tracer.ctx, C.byref(good), x, x, x, 1 << 31, x, None, None) == pkg.CRT_ERR_INVALID
    # nothing to do is CRT_OK and touches nothing
    assert L.crt_probe_rays_device(tracer.ctx, C.byref(good), 3, 0, None, None, None) == pkg.CRT_OK
    assert L.crt_probe_project_device(tracer.ctx, None, None, 0, 64, None, None) == pkg.CRT_OK
    assert L.crt_probe_validity_device(tracer.ctx, None, None, 0, 64, 0.5, None, None) == pkg.CRT_OK
    assert L.crt_probe_irradiance_device(tracer.ctx, C.byref(good), None, None, None, 0, None, None, None) == pkg.CRT_OK
    assert L.crt_probe_irradiance(tracer.ctx, C.byref(good), None, None, None, 0, None, None) == pkg.CRT_OK
    torch.cuda.synchronize()
    assert np.array_equal(tracer.read_quantized(), before) and bytes(tracer.stats()) == stats_before
    # a frame rendered before and after a bake is identical, and the bake leaves the colour buffer and the statistics alone
    tracer.bake_probes(pkg.make_probe_volume(**dict(v.fields(), backface_limit=0.5)))
    assert np.array_equal(tracer.read_quantized(), before) and bytes(tracer.stats()) == stats_before
    again = tracer.render(max_depth=3)
    assert np.array_equal(again.view(np.uint32), frame.view(np.uint32))


def lookup_points(rng, v, rec):
    """on probes, on the far faces, outside on every side, inside cells -- among them one with all eight and one with seven corners
    invalid, when the volume has such cells --, and with NaN and inf coordinates and normals"""
    n = np.array(v.n)
    span = v.spacing * (n - 1)
    far = v.origin + span
    outside = np.array([v.origin - 1.5, far + 1.5] + [np.where(np.arange(3) == k, side, v.origin + span / 2) for k in range(3)
                                                      for side in ((v.origin - 2.0)[k], (far + 2.0)[k])], dtype=F32)
    cell0 = (v.origin + v.spacing * np.array([0.4, 0.3, 0.6])).astype(F32)                     # inside cell (0, 0, 0)
    cell1 = (v.origin + v.spacing * np.array([1.4, 0.3, 0.6])).astype(F32)                     # inside cell (1, 0, 0)
    pts = np.concatenate([ps.positions(v, np.arange(v.count)), far[None, :], outside, cell0[None, :], cell1[None, :]]).astype(F32)
    return pts


@pytest.mark.parametrize("n", [1, 64, 65, 1000])
def test_probe_lookup_gives_the_rules_colours(pkg, world, n):
    import torch
    tracer = world["tracer"]
    rng = np.random.default_rng(n)
    seen = set()
    for dims in (dict(nx=3, ny=2, nz=4), dict(nx=1, ny=4, nz=1), dict(nx=1, ny=1, nz=1)):
        v = ps.Volume(rays=64, **dict(PLACE, **dims))
        rec = np.zeros(v.count, dtype=ps.PROBE_DTYPE)
        rec["coef"] = rng.uniform(-0.5, 2.0, (v.count, 9, 3)).astype(F32)
        rec["rays"] = 64
        rec["state"] = np.where((rng.uniform(size=v.count) < 0.25) & (np.arange(v.count) < 12), ps.INVALID, ps.VALID)   # (the upper cells stay whole)
        if v.n == (3, 2, 4):
            cell = [(iz * 2 + iy) * 3 + ix for iz in (0, 1) for iy in (0, 1) for ix in (0, 1)]
            rec["state"][cell] = ps.INVALID                                      # cell (0, 0, 0): all eight corners invalid
            nxt = [(iz * 2 + iy) * 3 + 2 for iz in (0, 1) for iy in (0, 1)]
            rec["state"][nxt] = [ps.VALID, ps.INVALID, ps.INVALID, ps.INVALID]   # cell (1, 0, 0): seven invalid
            rec["state"][-1] = 7                                                 # neither state: taken as INVALID
        fixed = lookup_points(rng, v, rec)
        span = np.maximum(v.spacing * (np.array(v.n) - 1), 1.0)
        if n < len(fixed):
            pts = fixed[rng.permutation(len(fixed))[:n]]
        else:                                                                    # the fixed points, then random ones in and around the volume
            pts = np.concatenate([fixed, (v.origin + rng.uniform(-0.2, 1.2, (n - len(fixed), 3)) * span).astype(F32)])
        nrm = rng.normal(size=pts.shape).astype(F32)
        if n >= 64:
            for k, value in enumerate([np.nan, np.inf, -np.inf]):
                pts[-1 - k, k] = value
                nrm[-4 - k, k] = value
        want_rgb, want_status = ps.lookup(v, rec, pts, nrm)
        d_rec, d_pts, d_nrm = Guarded(torch, rec.nbytes, rec), Guarded(torch, pts.nbytes, pts), Guarded(torch, nrm.nbytes, nrm)
        d_rgb, d_status = Guarded(torch, 12 * len(pts)), Guarded(torch, len(pts))
        vol = pkg.make_probe_volume(**v.fields())
        tracer.probe_irradiance_device(vol, d_rec.ptr(), d_pts.ptr(), d_nrm.ptr(), len(pts), d_rgb.ptr(), d_status.ptr())
        torch.cuda.synchronize()
        what = "%r, %d points" % (dims, len(pts))
        ps.same_colours(d_rgb.values(F32).reshape(-1, 3), want_rgb, what)
        assert np.array_equal(d_status.values(np.uint8), want_status), what
        assert all(g.intact() for g in (d_rec, d_pts, d_nrm, d_rgb, d_status)), what + ": a guard byte was written"
        # the host variant, and a call without a status array
        rgb, status = tracer.probe_irradiance(vol, rec, pts, nrm)
        ps.same_colours(rgb, want_rgb, what + ", host variant")
        assert np.array_equal(status, want_status)
        d_rgb.fill()
        tracer.probe_irradiance_device(vol, d_rec.ptr(), d_pts.ptr(), d_nrm.ptr(), len(pts), d_rgb.ptr(), None)
        torch.cuda.synchronize()
        ps.same_colours(d_rgb.values(F32).reshape(-1, 3), want_rgb, what + ", no status")
        if n >= 64:
            assert (want_status[-6:] == 0).all()
        seen |= set(want_status.tolist())
    if n == 1000:
        assert {0, 1, 2, 8} <= seen, seen


def test_the_all_invalid_and_seven_invalid_cells(pkg, world):
    """the two cells by name: no light in the one, one corner's light in the other"""
    tracer = world["tracer"]
    rng = np.random.default_rng(5)
    v = ps.Volume(rays=64, **dict(PLACE, nx=3, ny=2, nz=4))
    rec = np.zeros(v.count, dtype=ps.PROBE_DTYPE)
    rec["coef"] = rng.uniform(0.1, 2.0, (v.count, 9, 3)).astype(F32)
    rec["state"] = ps.VALID
    rec["state"][[(iz * 2 + iy) * 3 + ix for iz in (0, 1) for iy in (0, 1) for ix in (0, 1)]] = ps.INVALID
    rec["state"][[(iz * 2 + iy) * 3 + 2 for iz in (0, 1) for iy in (0, 1)][1:]] = ps.INVALID
    pts = np.array([v.origin + v.spacing * np.array([0.4, 0.3, 0.6]), v.origin + v.spacing * np.array([1.4, 0.3, 0.6])], dtype=F32)
    nrm = np.array([(0, 0, 1), (0, 0, 1)], dtype=F32)
    want_rgb, want_status = ps.lookup(v, rec, pts, nrm)
    assert want_status.tolist() == [0, 1]
    rgb, status = tracer.probe_irradiance(pkg.make_probe_volume(**v.fields()), rec, pts, nrm)
    ps.same_colours(rgb, want_rgb, "the two cells")
    assert status.tolist() == [0, 1] and not rgb[0].any()


def test_the_chain_in_a_stream_capture(pkg, world):
    """probe_rays, shoot_rays_enqueue, probe_project and probe_irradiance_device captured once and replayed twice: the rule's bytes"""
    import torch
    tracer, v = world["tracer"], world["volume"]
    vol = pkg.make_probe_volume(**v.fields())
    n = v.count * v.rays
    rays, rgb, probes = Guarded(torch, 24 * n), Guarded(torch, 12 * n), Guarded(torch, 128 * v.count)
    rng = np.random.default_rng(9)
    span = v.spacing * (np.array(v.n) - 1)
    pts = (v.origin + rng.uniform(-0.1, 1.1, (200, 3)) * span).astype(F32)
    nrm = rng.normal(size=pts.shape).astype(F32)
    d_pts, d_nrm, out, status = Guarded(torch, pts.nbytes, pts), Guarded(torch, nrm.nbytes, nrm), Guarded(torch, 12 * len(pts)), Guarded(torch, len(pts))
    # size the context's level arrays for these rays, outside the capture
    tracer.probe_rays_device(vol, 0, v.count, rays.ptr())
    tracer.shoot_rays_device(rays.ptr(), n, rgb.ptr())
    torch.cuda.synchronize()
    try:
        tracer.shoot_rays_enqueue(rays.ptr(), n, rgb.ptr())
    except pkg.CrtError as e:
        pytest.skip("crt_shoot_rays_enqueue refuses these sizes: %s" % e)
    tracer.shoot_stats()            # harvests the open call: a capture cannot wait for it
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stream = torch.cuda.current_stream().cuda_stream
        tracer.probe_rays_device(vol, 0, v.count, rays.ptr(), None, stream)
        tracer.shoot_rays_enqueue(rays.ptr(), n, rgb.ptr(), stream_ptr=stream)
        tracer.probe_project_device(rays.ptr(), rgb.ptr(), v.count, v.rays, probes.ptr(), stream)
        tracer.probe_irradiance_device(vol, probes.ptr(), d_pts.ptr(), d_nrm.ptr(), len(pts), out.ptr(), status.ptr(), stream)
    torch.cuda.synchronize()
    want_rgb, want_status = ps.lookup(v, world["records"], pts, nrm)
    for _ in range(2):
        for g in (rays, rgb, probes, out, status):
            g.fill()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(rays.values(U32), world["rays"].view(U32).ravel())
        ps.same_colours(rgb.values(F32).reshape(-1, 3), world["golden"], "a replay's colours")
        ps.same_records(probes.values(ps.PROBE_DTYPE), world["records"], "a replay's records")
        ps.same_colours(out.values(F32).reshape(-1, 3), want_rgb, "a replay's lookup")
        assert np.array_equal(status.values(np.uint8), want_status)
    assert all(g.intact() for g in (rays, rgb, probes, d_pts, d_nrm, out, status))
    del graph
