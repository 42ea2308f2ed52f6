"""The chunk loops of the ray, lighting and radiance queries (csrc/crt_query.hip: rays per round trip of the host variants, per launch,
per pass of a radiance query), which a few thousand rays never enter at their default sizes of 2^22, 2^27 and 2^22.  The test hook
Tracer.set_query_chunks lowers them to 1024, 192 and 1024 -- 192 is no multiple of the 256-thread workgroup and none of a wave's claim
-- so that 4096 rays are four host chunks of six launches each, the last launch partial.  Every answer is the CPU oracle's bit for
bit, and every statistic is what the same call reports with the default sizes."""
import numpy as np
import pytest

import query_sets as qs
import shade_sets as ss
import shoot_sets as sh
from helpers import assert_same_floats, assert_same_hits, assert_shaded, distances, level_rays, same_bits, small_case

pytestmark = pytest.mark.gpu
CHUNKS = dict(host_rays=1024, launch_rays=192, pass_rays=1024)
N = 4096
SHOOT_DEPTH = 2
_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def release_cases():
    """the tracers (GPU contexts with their scratch) live as long as this module's tests"""
    yield
    _CASES.clear()


def case(pkg, scenes, oracle, name, tmp_path_factory, tuning=None):
    """A scene's tracer and oracle, made once; what the oracle says of a ray set is added to it by the tests that need it (want)."""
    key = (name, tuple(sorted((tuning or {}).items())))
    if key not in _CASES:
        scene, depth, folder = small_case(scenes, name, tmp_path_factory.mktemp(name))
        tracer = pkg.Tracer(pkg.Scene(json_text=scenes.to_json(scene), folder=folder), tuning=pkg.make_tuning(**tuning) if tuning else None)
        _CASES[key] = dict(name=name, scene=scene, depth=depth, folder=folder, tracer=tracer, oracle=oracle.OracleScene(scenes.to_blob(scene)))
    return _CASES[key]


def want(c, what, make):
    if what not in c:
        c[what] = make()
        c[what].setflags(write=False)
    return c[what]


def random_wants(pkg, scenes, oracle, tmp_path_factory):
    """hw11, the 4096 random rays: the oracle's records as REFLECTION and PRIMARY rays and its occlusion within distances(n)"""
    c = case(pkg, scenes, oracle, "hw11", tmp_path_factory)
    rays = want(c, "rays", qs.random_rays)
    assert len(rays) == N
    for ray_type in (qs.RAY_REFLECTION, qs.RAY_PRIMARY):
        want(c, "hits%d" % ray_type, lambda: qs.oracle_hits(c["oracle"], c["scene"], rays, ray_type, pkg.HIT_DTYPE))
    want(c, "dist", lambda: distances(N))
    want(c, "occ", lambda: qs.oracle_occluded(c["oracle"], rays, c["dist"]))
    return c


def query_tuple(st):
    return (int(st.rays), int(st.hits), int(st.rerouted))


def shoot_tuple(st):
    return (int(st.rays), int(st.levels), [int(x) for x in st.level_rays], int(st.shadow_records), int(st.rerouted))


def closest_in_chunks(pkg, c, tracer, rays, ray_type, want_hits, what):
    """trace_rays with the default sizes, then in chunks: the oracle's records both times, and the same statistics"""
    got = tracer.trace_rays(rays, ray_type)
    dflt = query_tuple(tracer.query_stats())
    assert_same_hits(got, want_hits, what + ", default sizes")
    assert dflt[:2] == (len(rays), int(want_hits["hit"].sum()))
    tracer.set_query_chunks(**CHUNKS)
    got = tracer.trace_rays(rays, ray_type)
    st = query_tuple(tracer.query_stats())
    print("%s: rays %d hits %d rerouted %d (default sizes: %d)" % (what, st[0], st[1], st[2], dflt[2]))
    assert_same_hits(got, want_hits, what + ", in chunks")
    assert st == dflt, what
    return st


def occluded_in_chunks(tracer, rays, dist, want_occ, what):
    got = tracer.occluded_rays(rays, dist)
    dflt = query_tuple(tracer.query_stats())
    assert np.array_equal(got, want_occ), what + ", default sizes"
    assert dflt[:2] == (len(rays), int(want_occ.sum()))
    tracer.set_query_chunks(**CHUNKS)
    got = tracer.occluded_rays(rays, dist)
    st = query_tuple(tracer.query_stats())
    print("%s: rays %d occluded %d rerouted %d (default sizes: %d)" % (what, st[0], st[1], st[2], dflt[2]))
    bad = np.flatnonzero(got != want_occ)
    assert bad.size == 0, "%s, in chunks: %d rays differ, first %d" % (what, bad.size, bad[0])
    assert st == dflt, what
    return st


def closest_and_occluded(pkg, c):
    tracer = c["tracer"]
    try:
        for ray_type in (qs.RAY_REFLECTION, qs.RAY_PRIMARY):
            tracer.set_query_chunks()
            closest_in_chunks(pkg, c, tracer, c["rays"], ray_type, c["hits%d" % ray_type], "hw11 type %d" % ray_type)
        tracer.set_query_chunks()
        occluded_in_chunks(tracer, c["rays"], c["dist"], c["occ"], "hw11 per-ray distances")
    finally:
        tracer.set_query_chunks()


# ---- 1. ray queries: four host chunks of six launches
def test_ray_queries_in_chunks(pkg, scenes, oracle, tmp_path_factory):
    closest_and_occluded(pkg, random_wants(pkg, scenes, oracle, tmp_path_factory))


# ---- 2. the reroute list, launch by launch
def test_in_plane_rays_reroute_the_same_sum_over_24_launches(pkg, scenes, oracle, tmp_path_factory):
    c = case(pkg, scenes, oracle, "hw11", tmp_path_factory)
    rays = want(c, "in_plane", lambda: np.ascontiguousarray(np.resize(qs.in_plane_rays(c["scene"]), (N, 6))))
    want_hits = want(c, "in_plane_hits", lambda: qs.oracle_hits(c["oracle"], c["scene"], rays, qs.RAY_REFLECTION, pkg.HIT_DTYPE))
    tracer = c["tracer"]
    try:
        tracer.set_query_chunks()
        st = closest_in_chunks(pkg, c, tracer, rays, qs.RAY_REFLECTION, want_hits, "hw11 in-plane")
        assert st[2] == qs.non_finite_winners(want_hits) > 0
        tracer.set_query_chunks()
        occluded_in_chunks(tracer, rays, np.float32(np.inf), want(c, "in_plane_occ", lambda: qs.oracle_occluded(c["oracle"], rays, np.float32(np.inf))),
                           "hw11 in-plane, no limit")
    finally:
        tracer.set_query_chunks()


# ---- 3. without the filter: every launch is the reroute kernel's
def test_without_the_filter_every_ray_of_every_launch_is_rerouted(pkg, scenes, oracle, tmp_path_factory):
    c = random_wants(pkg, scenes, oracle, tmp_path_factory)
    tracer = case(pkg, scenes, oracle, "hw11", tmp_path_factory, tuning=dict(bvh=0))["tracer"]
    try:
        tracer.set_query_chunks()
        assert closest_in_chunks(pkg, c, tracer, c["rays"], qs.RAY_REFLECTION, c["hits%d" % qs.RAY_REFLECTION], "bvh=0")[2] == N
        tracer.set_query_chunks()
        assert occluded_in_chunks(tracer, c["rays"], c["dist"], c["occ"], "bvh=0 occlusion")[2] == N
    finally:
        tracer.set_query_chunks()


# ---- 4. direct lighting of those records
def shade_wants(pkg, scenes, oracle, tmp_path_factory):
    """The oracle's colours of the random rays' records (compared where shoot_ray's normalisation leaves the direction alone:
    tests/shade_sets.py), their status, and the light sums of the DIFFUSE ones on a white surface."""
    c = random_wants(pkg, scenes, oracle, tmp_path_factory)
    hits = c["hits%d" % qs.RAY_REFLECTION]
    want(c, "fixed", lambda: ss.is_fixed_point(c["rays"]))
    want(c, "status", lambda: ss.expected_status(pkg, c["scene"], hits))
    want(c, "colours", lambda: ss.oracle_colours(c["oracle"], c["rays"]))
    diffuse = c["status"] == pkg.SHADE_DIFFUSE
    white = oracle.OracleScene(scenes.to_blob(ss.white_scene(c["scene"])))
    want(c, "light", lambda: ss.oracle_colours(white, c["rays"][diffuse])[:, 0].copy())
    return c, hits, diffuse


def test_direct_lighting_in_chunks(pkg, scenes, oracle, tmp_path_factory):
    c, hits, diffuse = shade_wants(pkg, scenes, oracle, tmp_path_factory)
    tracer, fixed = c["tracer"], c["fixed"]
    n_diffuse = int(diffuse.sum())
    assert int(fixed.sum()) >= 1000 and n_diffuse >= 1200
    points, normals = hits["point"][diffuse].copy(), hits["normal"][diffuse].copy()
    try:
        tracer.set_query_chunks()
        rgb0, status0 = tracer.shade_hits(hits)
        dflt = query_tuple(tracer.query_stats())
        light0 = tracer.light_points(points, normals)
        dflt_light = query_tuple(tracer.query_stats())
        tracer.set_query_chunks(**CHUNKS)
        rgb, status = tracer.shade_hits(hits)
        st = query_tuple(tracer.query_stats())
        light = tracer.light_points(points, normals)
        st_light = query_tuple(tracer.query_stats())
    finally:
        tracer.set_query_chunks()
    print("shade_hits: records %d diffuse %d rerouted %d; light_points: %d rerouted %d" % (st[0], st[1], st[2], st_light[0], st_light[2]))
    assert_shaded(pkg, rgb[fixed], status[fixed], c["status"][fixed], c["colours"][fixed], "shade_hits in chunks")
    assert np.array_equal(status, c["status"])
    assert_same_floats(rgb, rgb0, "shade_hits in chunks against the default sizes")
    assert np.array_equal(status, status0)
    assert st == dflt and st[:2] == (N, n_diffuse)
    assert_same_floats(light[fixed[diffuse]], c["light"][fixed[diffuse]], "light_points in chunks")
    assert_same_floats(light, light0, "light_points in chunks against the default sizes")
    assert st_light == dflt_light and st_light[:2] == (n_diffuse, n_diffuse)


# ---- 5. radiance queries: passes, levels, launches
def shoot_case(pkg, scenes, oracle, name, tmp_path_factory):
    c = case(pkg, scenes, oracle, name, tmp_path_factory)
    rays = want(c, "shoot_rays", lambda: sh.rays_for(name, c["scene"]))
    want(c, "shoot_colours", lambda: sh.oracle_colours(c["oracle"], rays, SHOOT_DEPTH))
    return c, rays


@pytest.mark.parametrize("name", ["hw11", "hw14"])
def test_radiance_queries_in_chunks(pkg, scenes, oracle, name, tmp_path_factory):
    c, rays = shoot_case(pkg, scenes, oracle, name, tmp_path_factory)
    tracer = c["tracer"]
    try:
        tracer.set_query_chunks()
        rgb0 = tracer.shoot_rays(rays, max_depth=SHOOT_DEPTH)
        dflt, qdflt = shoot_tuple(tracer.shoot_stats()), query_tuple(tracer.query_stats())
        tracer.set_query_chunks(**CHUNKS)
        rgb = tracer.shoot_rays(rays, max_depth=SHOOT_DEPTH)
        st, qst = shoot_tuple(tracer.shoot_stats()), query_tuple(tracer.query_stats())
    finally:
        tracer.set_query_chunks()
    print("%s: rays %d levels %d level_rays %s shadow_records %d rerouted %d; query stats %s" % (name, st[0], st[1], st[2][:st[1]], st[3], st[4], qst))
    assert_same_floats(rgb0, c["shoot_colours"], name + ", default sizes")
    assert_same_floats(rgb, c["shoot_colours"], name + ", in chunks")
    assert st[0] == len(rays) == st[2][0] and st[2][1] > 0, "the set must reach level 1"
    assert st == dflt and qst == qdflt and qst[0] == len(rays) and qst[2] == st[4]


# ---- 6. the device variants, 22 launches a call, on a stream of the test's own
def device_arrays(pkg, c, hits, diffuse, shoot_rays):
    import torch
    n, m = len(hits), int(diffuse.sum())
    return dict(rays=torch.from_numpy(np.array(c["rays"])).cuda(), dist=torch.from_numpy(np.array(c["dist"])).cuda(),
                records=torch.from_numpy(np.ascontiguousarray(hits).view(np.uint8).reshape(n, 48).copy()).cuda(),
                points=torch.from_numpy(hits["point"][diffuse].copy()).cuda(), normals=torch.from_numpy(hits["normal"][diffuse].copy()).cuda(),
                shoot=torch.from_numpy(np.array(shoot_rays)).cuda(),
                hits=torch.full((n + 1, 48), 0xA5, dtype=torch.uint8, device="cuda"),      # (one record more: must stay untouched)
                occ=torch.full((n + 1,), 0xA5, dtype=torch.uint8, device="cuda"),
                rgb=torch.full((n + 1, 3), float("nan"), dtype=torch.float32, device="cuda"),
                status=torch.full((n + 1,), 0xA5, dtype=torch.uint8, device="cuda"),
                light=torch.full((m + 1,), float("nan"), dtype=torch.float32, device="cuda"),
                colours=torch.full((len(shoot_rays) + 1, 3), float("nan"), dtype=torch.float32, device="cuda"))


def test_device_variants_in_chunks(pkg, scenes, oracle, tmp_path_factory):
    import torch
    c, hits, diffuse = shade_wants(pkg, scenes, oracle, tmp_path_factory)
    _, shoot_rays = shoot_case(pkg, scenes, oracle, "hw11", tmp_path_factory)
    tracer, fixed, m, k = c["tracer"], c["fixed"], int(diffuse.sum()), len(shoot_rays)
    d = device_arrays(pkg, c, hits, diffuse, shoot_rays)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    try:
        tracer.set_query_chunks(launch_rays=CHUNKS["launch_rays"])
        with torch.cuda.stream(stream):
            s = stream.cuda_stream
            tracer.trace_rays_device(d["rays"].data_ptr(), N, qs.RAY_REFLECTION, d["hits"].data_ptr(), s)
            assert query_tuple(tracer.query_stats()) == (N, int(hits["hit"].sum()), 0)
            tracer.occluded_rays_device(d["rays"].data_ptr(), d["dist"].data_ptr(), N, d["occ"].data_ptr(), s)
            assert query_tuple(tracer.query_stats()) == (N, int(c["occ"].sum()), 0)
            tracer.shade_hits_device(d["records"].data_ptr(), N, d["rgb"].data_ptr(), d["status"].data_ptr(), stream_ptr=s)
            assert query_tuple(tracer.query_stats())[:2] == (N, m)
            tracer.light_points_device(d["points"].data_ptr(), d["normals"].data_ptr(), m, d["light"].data_ptr(), stream_ptr=s)
            assert query_tuple(tracer.query_stats())[:2] == (m, m)
            tracer.shoot_rays_device(d["shoot"].data_ptr(), k, d["colours"].data_ptr(), max_depth=SHOOT_DEPTH, stream_ptr=s)
            st = shoot_tuple(tracer.shoot_stats())
        stream.synchronize()
        tracer.set_query_chunks()
        tracer.shoot_rays(shoot_rays, max_depth=SHOOT_DEPTH)
        assert st == shoot_tuple(tracer.shoot_stats())
    finally:
        tracer.set_query_chunks()
    got = {name: d[name].cpu().numpy() for name in ("hits", "occ", "rgb", "status", "light", "colours")}
    assert np.all(got["hits"][N:] == 0xA5) and got["occ"][N] == 0xA5 and np.all(np.isnan(got["rgb"][N:])) and got["status"][N] == 0xA5
    assert np.isnan(got["light"][m]) and np.all(np.isnan(got["colours"][k:])), "written past the end"
    assert_same_hits(got["hits"][:N].view(pkg.HIT_DTYPE).reshape(-1), hits, "trace_rays_device in launches of 192")
    assert np.array_equal(got["occ"][:N].astype(bool), c["occ"]), "occluded_rays_device in launches of 192"
    assert np.array_equal(got["status"][:N], c["status"])
    assert_shaded(pkg, got["rgb"][:N][fixed], got["status"][:N][fixed], c["status"][fixed], c["colours"][fixed], "shade_hits_device in launches of 192")
    assert_same_floats(got["light"][:m][fixed[diffuse]], c["light"][fixed[diffuse]], "light_points_device in launches of 192")
    assert_same_floats(got["colours"][:k], c["shoot_colours"], "shoot_rays_device in launches of 192")


# ---- 7. four calls on two streams, nothing read in between
def test_interleaved_calls_on_two_streams(pkg, scenes, oracle, tmp_path_factory):
    import torch
    c, hits, diffuse = shade_wants(pkg, scenes, oracle, tmp_path_factory)
    _, shoot_rays = shoot_case(pkg, scenes, oracle, "hw11", tmp_path_factory)
    tracer, fixed, depth, k = c["tracer"], c["fixed"], c["depth"], len(shoot_rays)
    frame0 = tracer.render(max_depth=depth).copy()
    tracer.shoot_rays(shoot_rays, max_depth=SHOOT_DEPTH)
    alone = shoot_tuple(tracer.shoot_stats())
    d = device_arrays(pkg, c, hits, diffuse, shoot_rays)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    try:
        tracer.set_query_chunks(**CHUNKS)
        tracer.trace_rays_device(d["rays"].data_ptr(), N, qs.RAY_REFLECTION, d["hits"].data_ptr(), a.cuda_stream)
        tracer.shade_hits_device(d["records"].data_ptr(), N, d["rgb"].data_ptr(), d["status"].data_ptr(), stream_ptr=b.cuda_stream)
        tracer.shoot_rays_device(d["shoot"].data_ptr(), k, d["colours"].data_ptr(), max_depth=SHOOT_DEPTH, stream_ptr=a.cuda_stream)
        tracer.occluded_rays_device(d["rays"].data_ptr(), d["dist"].data_ptr(), N, d["occ"].data_ptr(), b.cuda_stream)
        a.synchronize()
        b.synchronize()
        # include/crt_hip.h: the last query call's, the last radiance call's
        assert query_tuple(tracer.query_stats()) == (N, int(c["occ"].sum()), 0)
        assert shoot_tuple(tracer.shoot_stats()) == alone
    finally:
        tracer.set_query_chunks()
    got = {name: d[name].cpu().numpy() for name in ("hits", "occ", "rgb", "status", "colours")}
    assert_same_hits(got["hits"][:N].view(pkg.HIT_DTYPE).reshape(-1), hits, "trace_rays_device on stream A")
    assert np.array_equal(got["status"][:N], c["status"])
    assert_shaded(pkg, got["rgb"][:N][fixed], got["status"][:N][fixed], c["status"][fixed], c["colours"][fixed], "shade_hits_device on stream B")
    assert_same_floats(got["colours"][:k], c["shoot_colours"], "shoot_rays_device on stream A")
    assert np.array_equal(got["occ"][:N].astype(bool), c["occ"]), "occluded_rays_device on stream B"
    assert_same_floats(tracer.render(max_depth=depth), frame0, "the frame after the queries")


# ---- 8. the same with enqueue calls among them: six calls on two streams, one of them the enqueue call that does not wait
def test_interleaved_enqueue_calls_on_two_streams(pkg, scenes, oracle, tmp_path_factory):
    import ctypes as C
    import torch
    c, hits, diffuse = shade_wants(pkg, scenes, oracle, tmp_path_factory)
    _, shoot_rays = shoot_case(pkg, scenes, oracle, "hw11", tmp_path_factory)
    tracer, depth, k = c["tracer"], c["depth"], len(shoot_rays)
    frame0 = tracer.render(max_depth=depth).copy()
    d = device_arrays(pkg, c, hits, diffuse, shoot_rays)
    tracer.shoot_rays_device(d["shoot"].data_ptr(), k, d["colours"].data_ptr(), max_depth=SHOOT_DEPTH)   # alone: the yardstick (and the scratch's size)
    torch.cuda.synchronize()
    alone, alone_hits = tracer.shoot_stats(), int(tracer.query_stats().hits)
    sync = d["colours"].cpu().numpy()[:k].copy()
    lr = level_rays(alone)
    print("hw11 at depth %d: level_rays %s" % (SHOOT_DEPTH, lr[:alone.levels]))
    assert lr[1] > 0 and any(n > 256 for n in lr[1:alone.levels]), "condition on the input: a level below level 0 in several launches"
    d["colours"].fill_(float("nan"))
    rgb = [torch.full((k + 1, 3), float("nan"), dtype=torch.float32, device="cuda") for _ in range(3)]
    rep = [torch.full((C.sizeof(pkg.ShootReport),), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(3)]
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()

    def enqueue(i):
        tracer.shoot_rays_enqueue(d["shoot"].data_ptr(), k, rgb[i].data_ptr(), max_depth=SHOOT_DEPTH, d_report_ptr=rep[i].data_ptr(), stream_ptr=a.cuda_stream)

    try:
        tracer.set_query_chunks(launch_rays=256)
        enqueue(0)
        tracer.trace_rays_device(d["rays"].data_ptr(), N, qs.RAY_REFLECTION, d["hits"].data_ptr(), b.cuda_stream)
        enqueue(1)
        enqueue(2)   # behind an enqueue call on its stream: the call that does not wait
        tracer.shoot_rays_device(d["shoot"].data_ptr(), k, d["colours"].data_ptr(), max_depth=SHOOT_DEPTH, stream_ptr=b.cuda_stream)
        tracer.occluded_rays_device(d["rays"].data_ptr(), d["dist"].data_ptr(), N, d["occ"].data_ptr(), a.cuda_stream)
        a.synchronize()
        b.synchronize()
        assert shoot_tuple(tracer.shoot_stats()) == shoot_tuple(alone)
        assert query_tuple(tracer.query_stats()) == (N, int(c["occ"].sum()), 0)
    finally:
        tracer.set_query_chunks()
    for i in range(3):
        got = rgb[i].cpu().numpy()
        assert np.all(np.isnan(got[k:])), "written past the end"
        same_bits(got[:k], sync, "enqueue call %d on stream A" % i)
        r = pkg.ShootReport.from_buffer_copy(rep[i].cpu().numpy().tobytes())
        assert (r.levels, level_rays(r), r.shadow_records, r.rerouted, r.hits) == (alone.levels, lr, alone.shadow_records, alone.rerouted, alone_hits), i
        assert (r.overflow, r.dropped) == (0, 0), i
    got = {name: d[name].cpu().numpy() for name in ("hits", "occ", "colours")}
    assert_same_hits(got["hits"][:N].view(pkg.HIT_DTYPE).reshape(-1), hits, "trace_rays_device on stream B")
    same_bits(got["colours"][:k], sync, "shoot_rays_device on stream B")
    assert_same_floats(got["colours"][:k], c["shoot_colours"], "shoot_rays_device on stream B: the oracle's colours")
    assert np.array_equal(got["occ"][:N].astype(bool), c["occ"]), "occluded_rays_device on stream A"
    assert_same_floats(tracer.render(max_depth=depth), frame0, "the frame after the queries")


# ---- 9. zeros restore the defaults: the staging arrays grow back
def test_zeros_restore_the_defaults(pkg, scenes, oracle, tmp_path_factory):
    c = random_wants(pkg, scenes, oracle, tmp_path_factory)
    tracer = pkg.Tracer(pkg.Scene(json_text=scenes.to_json(c["scene"]), folder=c["folder"]))   # (a context whose first call is a small one)
    fresh = dict(c, tracer=tracer)
    try:
        tracer.set_query_chunks(**CHUNKS)
        assert_same_hits(tracer.trace_rays(c["rays"], qs.RAY_REFLECTION), c["hits%d" % qs.RAY_REFLECTION], "in chunks, first call of the context")
        tracer.set_query_chunks(1, 1, 1)               # clamped to 64
        assert_same_hits(tracer.trace_rays(c["rays"][:200], qs.RAY_REFLECTION), c["hits%d" % qs.RAY_REFLECTION][:200], "chunks of 64")
        tracer.set_query_chunks(2 ** 40, 2 ** 40, 2 ** 40)   # clamped to the defaults
        tracer.set_query_chunks()
        closest_and_occluded(pkg, fresh)
    finally:
        tracer.set_query_chunks()
