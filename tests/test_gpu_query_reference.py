"""The ray, lighting and radiance queries on the GPU (include/crt_hip.h: crt_trace_rays*, crt_occluded_rays*, crt_shade_hits*,
crt_shoot_rays*, crt_shoot_rays_enqueue) against the REAL reference's own intersect, checkForIntersection and shootRay: the fixtures
tests/golden/query_<scene>.npz (tests/reference_ray_sets.py).  Every comparison is bit for bit (NaN equals NaN); nothing but
tests/golden/ is read.  One Tracer per scene and tuning, made once."""
import ctypes as C

import numpy as np
import pytest

import query_sets as qs
import reference_ray_sets as rrs
from degenerate_sets import normalized
from helpers import assert_same_floats, assert_same_hits, assert_shaded, blob_to_scene, same_bits

pytestmark = pytest.mark.gpu
# default tuning; the reference-order walk for every ray; the filter walks with 4 stack entries (tests/test_gpu_filter_rare.py)
VARIANTS = ["default", "bvh0", "stack4"]
TYPE_IDS = ["primary", "shadow", "reflection", "refraction"]
# scenes known to keep the candidate filter with room for a lowered stack; at these details the library builds none for hw14 and hw12, and
# `mixed` has ill-formed triangles
HAS_FILTER = ["hw11"]
# the lowered stack is a property of the filter walks: only where the scene has a filter (that the setter acts -- rays rerouted when the
# stack runs out -- is tests/test_gpu_filter_rare.py::test_a_full_stack_reroutes_query_rays)
CASES = [(name, variant) for name in rrs.SCENES for variant in VARIANTS if variant != "stack4" or name in HAS_FILTER]
_tracers = {}


@pytest.fixture(scope="module")
def tracer_of(pkg, scenes, tmp_path_factory):
    def get(name, variant="default"):
        key = (name, variant)
        if key not in _tracers:
            scene = blob_to_scene(rrs.load_fixture(name)[0])
            folder = ""
            if scene.get("textures"):
                folder = str(tmp_path_factory.mktemp("query_reference_bitmaps"))
                scenes.write_bitmaps(scene, folder)
            tuning = pkg.make_tuning(bvh=0) if variant == "bvh0" else None
            t = pkg.Tracer(pkg.Scene(json_text=scenes.to_json(scene), folder=folder), tuning=tuning)
            if variant == "stack4":
                t.set_filter_stack(4)
            _tracers[key] = (t, scene)
        return _tracers[key]
    yield get
    for t, _ in _tracers.values():
        t.close()
    _tracers.clear()


def rows_of(rs, cls):
    return np.flatnonzero(rs["labels"] == rrs.CLASSES.index(cls))


def as_pkg_hits(pkg, hits):
    assert pkg.HIT_DTYPE.itemsize == rrs.HIT_DTYPE.itemsize == 48
    return np.ascontiguousarray(hits).view(pkg.HIT_DTYPE)


# ---- 1. closest hits
@pytest.mark.parametrize("ray_type", rrs.RAY_TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("cls", rrs.CLASSES)
@pytest.mark.parametrize("name,variant", CASES)
def test_trace_rays_equal_the_reference(pkg, tracer_of, name, variant, cls, ray_type):
    _, rs, ans = rrs.load_fixture(name)
    tracer, _ = tracer_of(name, variant)
    rows = rows_of(rs, cls)
    if len(rows) == 0:
        assert name not in rrs.FULL_SCENES and cls in ("inside", "through_glass")
        return
    want = as_pkg_hits(pkg, ans["hits"][ray_type][rows])
    got = tracer.trace_rays(rs["rays"][rows], ray_type)
    st = tracer.query_stats()
    what = "%s %s %s type %d" % (name, variant, cls, ray_type)
    print("%s: rays %d hits %d (reference %d) rerouted %d non-finite winners %d" % (what, st.rays, st.hits, int(want["hit"].sum()), st.rerouted,
                                                                                   qs.non_finite_winners(want)))
    assert_same_hits(got, want, what)
    assert (st.rays, st.hits) == (len(rows), int(want["hit"].sum())), what
    # the routes are shown to run: a direction not of unit length and a refuted miss go to the reference-order walk, a random ray does not
    if variant == "bvh0" or cls == "scaled":
        assert st.rerouted == len(rows), what
    elif cls == "in_plane" and ray_type != qs.RAY_PRIMARY:
        # (a primary in-plane ray has n . d = 0 >= 0 for every triangle of its plane and is culled, Ray.cpp:13: no winner at t = NaN /
        # inf, no refuted miss, nothing to reroute -- tests/test_gpu_query_rays.py pins that count to 0)
        assert st.rerouted > 0 and st.rerouted >= qs.non_finite_winners(want), what
    elif cls == "random" and variant == "default" and name in HAS_FILTER:
        assert st.rerouted == 0, what


# ---- 2. occlusion at the caller's distances
@pytest.mark.parametrize("name,variant", CASES)
def test_occluded_rays_equal_the_reference(tracer_of, name, variant):
    _, rs, ans = rrs.load_fixture(name)
    tracer, _ = tracer_of(name, variant)
    scaled = rs["labels"][rs["occ_index"]] == rrs.CLASSES.index("scaled")
    assert scaled.sum() >= 100 and (~scaled).sum() >= 100
    for part, what in ((~scaled, "unit directions"), (scaled, "scaled directions")):
        idx = np.flatnonzero(part)
        got = tracer.occluded_rays(rs["rays"][rs["occ_index"][idx]], rs["occ_dist"][idx])
        st = tracer.query_stats()
        bad = idx[got != ans["occ"][idx]]
        assert bad.size == 0, "%s %s %s: %d of %d pairs differ, first: ray %d distance %r (%s)" % (
            name, variant, what, bad.size, len(idx), rs["occ_index"][bad[0]], rs["occ_dist"][bad[0]], rrs.OCC_KINDS[rs["occ_kind"][bad[0]]])
        assert (st.rays, st.hits) == (len(idx), int(ans["occ"][idx].sum()))
        if part is scaled or variant == "bvh0":
            assert st.rerouted == len(idx)


# ---- 3. radiance
@pytest.mark.parametrize("depth", rrs.DEPTHS)
@pytest.mark.parametrize("ray_type", rrs.RAY_TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("name,variant", CASES)
def test_shoot_rays_equal_the_reference(tracer_of, name, variant, ray_type, depth):
    _, rs, ans = rrs.load_fixture(name)
    tracer, _ = tracer_of(name, variant)
    # reference_ray_sets.DEEP_SCENES: not evaluated for the non-finite winners of the two deep scenes
    keep = np.flatnonzero(~ans["shoot_skip"]) if ray_type != qs.RAY_PRIMARY else np.arange(len(rs["rays"]))
    got = tracer.shoot_rays(rs["rays"][keep], ray_type, max_depth=depth)
    want = ans["shoot"][(ray_type, depth)][keep]
    for cls in rrs.CLASSES:                     # one call, compared class by class so that a failure names the class
        rows = np.flatnonzero(rs["labels"][keep] == rrs.CLASSES.index(cls))
        assert_same_floats(got[rows], want[rows], "%s %s %s type %d depth %d" % (name, variant, cls, ray_type, depth))


@pytest.mark.parametrize("name", rrs.SCENES)
def test_shoot_rays_enqueue_equals_the_reference(pkg, tracer_of, name):
    import torch
    _, rs, ans = rrs.load_fixture(name)
    tracer, _ = tracer_of(name)
    keep = np.flatnonzero(~ans["shoot_skip"])       # (reference_ray_sets.DEEP_SCENES)
    n = len(keep)
    d_rays = torch.from_numpy(np.ascontiguousarray(rs["rays"][keep])).cuda()
    d_rgb = torch.full((n + 1, 3), float("nan"), dtype=torch.float32, device="cuda")
    d_rep = torch.full((C.sizeof(pkg.ShootReport),), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for ray_type in (qs.RAY_PRIMARY, qs.RAY_REFLECTION):
        for depth in (5, 1, 0):                 # the deepest first: that synchronous call sizes the levels
            tracer.shoot_rays_device(d_rays.data_ptr(), n, d_rgb.data_ptr(), ray_type, max_depth=depth)
            torch.cuda.synchronize()
            assert_same_floats(d_rgb.cpu().numpy()[:n], ans["shoot"][(ray_type, depth)][keep], "%s synchronous type %d depth %d" % (name, ray_type, depth))
            d_rgb.fill_(float("nan"))
            torch.cuda.synchronize()
            tracer.shoot_rays_enqueue(d_rays.data_ptr(), n, d_rgb.data_ptr(), ray_type, max_depth=depth, d_report_ptr=d_rep.data_ptr())
            torch.cuda.synchronize()
            rep = pkg.ShootReport.from_buffer_copy(d_rep.cpu().numpy().tobytes())
            rgb = d_rgb.cpu().numpy()
            assert (rep.overflow, rep.dropped) == (0, 0) and np.all(np.isnan(rgb[n:]))
            assert_same_floats(rgb[:n], ans["shoot"][(ray_type, depth)][keep], "%s enqueue type %d depth %d" % (name, ray_type, depth))


# ---- 4. direct lighting of the reference's own hit records
@pytest.mark.parametrize("ray_type", rrs.RAY_TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("name,variant", CASES)
def test_shade_hits_equal_the_reference(pkg, tracer_of, name, variant, ray_type):
    """shootRay normalises the direction before it traces (RayTracer.cpp:420), intersect does not: the fixture's hit record is
    shootRay's own hit only for a ray whose direction that normalisation leaves as it is, bit for bit.  Those rays' colours are
    compared wherever the record is final; the status is checked for every record."""
    _, rs, ans = rrs.load_fixture(name)
    tracer, scene = tracer_of(name, variant)
    hits = as_pkg_hits(pkg, ans["hits"][ray_type])
    kinds = rrs.material_kinds(scene)[np.where(hits["hit"] == 1, hits["mesh"], 0)]
    status = np.where(hits["hit"] == 0, pkg.SHADE_BACKGROUND, np.where(kinds == "diffuse", pkg.SHADE_DIFFUSE,
                      np.where(kinds == "constant", pkg.SHADE_BACKGROUND, pkg.SHADE_RECURSES))).astype(np.uint8)
    same_direction = (normalized(rs["rays"][:, 3:]).view(np.uint32) == rs["rays"][:, 3:].view(np.uint32)).all(axis=1)
    # the length of most float32-rounded unit vectors rounds to exactly 1: the restriction keeps at least half of every class but `scaled`
    for k, cls in enumerate(rrs.CLASSES):
        rows = rs["labels"] == k
        if cls != "scaled" and rows.any():
            assert same_direction[rows].mean() >= 0.5, cls
    final = (status != pkg.SHADE_RECURSES) & same_direction
    assert final.sum() >= 300
    if name in rrs.FULL_SCENES:      # (in tie_ba the winner of every tie is the mirror quad)
        assert (final & (status == pkg.SHADE_DIFFUSE)).sum() >= 100
    keep = np.flatnonzero(~ans["shoot_skip"]) if ray_type != qs.RAY_PRIMARY else np.arange(len(hits))   # (reference_ray_sets.DEEP_SCENES)
    rgb, got_status = tracer.shade_hits(hits[keep])
    want, status, final = ans["shoot"][(ray_type, 0)][keep], status[keep], final[keep]
    bad = np.flatnonzero(got_status != status)
    assert bad.size == 0, "%s: status differs for %d records, first %d" % (name, bad.size, bad[0])
    assert_shaded(pkg, rgb[final], got_status[final], status[final], want[final], "%s %s type %d" % (name, variant, ray_type))


# ---- 5. the chunk loops and the device variants, on one scene
def test_chunks_of_64_rays(pkg, tracer_of):
    """class boundaries fall inside the chunks: the whole list in one call, 64 rays per round trip, launch and pass"""
    _, rs, ans = rrs.load_fixture("hw11")
    tracer, _ = tracer_of("hw11")
    tracer.set_query_chunks(64, 64, 64)
    try:
        for t in (qs.RAY_PRIMARY, qs.RAY_REFLECTION):
            assert_same_hits(tracer.trace_rays(rs["rays"], t), as_pkg_hits(pkg, ans["hits"][t]), "chunks of 64, type %d" % t)
            assert tracer.query_stats().rays == len(rs["rays"])
            assert_same_floats(tracer.shoot_rays(rs["rays"], t, max_depth=5), ans["shoot"][(t, 5)], "chunks of 64, shoot type %d" % t)
        got = tracer.occluded_rays(rs["rays"][rs["occ_index"]], rs["occ_dist"])
        assert np.array_equal(got, ans["occ"]), "chunks of 64, occlusion"
    finally:
        tracer.set_query_chunks()


def test_device_variants_on_a_stream_of_their_own(pkg, tracer_of):
    import torch
    _, rs, ans = rrs.load_fixture("hw11")
    tracer, _ = tracer_of("hw11")
    n, m = len(rs["rays"]), len(rs["occ_index"])
    d_rays = torch.from_numpy(np.array(rs["rays"])).cuda()
    d_occ_rays = torch.from_numpy(np.ascontiguousarray(rs["rays"][rs["occ_index"]])).cuda()
    d_dist = torch.from_numpy(np.array(rs["occ_dist"])).cuda()
    d_hits = torch.full((n + 1, 48), 0xA5, dtype=torch.uint8, device="cuda")
    d_occ = torch.full((m + 1,), 0xA5, dtype=torch.uint8, device="cuda")
    d_rgb = torch.full((n + 1, 3), float("nan"), dtype=torch.float32, device="cuda")
    d_shade = torch.full((n + 1, 3), float("nan"), dtype=torch.float32, device="cuda")
    d_status = torch.full((n + 1,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    t = qs.RAY_REFLECTION
    with torch.cuda.stream(stream):
        tracer.trace_rays_device(d_rays.data_ptr(), n, t, d_hits.data_ptr(), stream.cuda_stream)
        tracer.shade_hits_device(d_hits.data_ptr(), n, d_shade.data_ptr(), d_status.data_ptr(), stream_ptr=stream.cuda_stream)
        tracer.occluded_rays_device(d_occ_rays.data_ptr(), d_dist.data_ptr(), m, d_occ.data_ptr(), stream.cuda_stream)
        tracer.shoot_rays_device(d_rays.data_ptr(), n, d_rgb.data_ptr(), t, max_depth=5, stream_ptr=stream.cuda_stream)
    stream.synchronize()
    hits, occ, rgb = d_hits.cpu().numpy(), d_occ.cpu().numpy(), d_rgb.cpu().numpy()
    assert np.all(hits[n:] == 0xA5) and np.all(occ[m:] == 0xA5) and np.all(np.isnan(rgb[n:])), "written past the end"
    assert_same_hits(hits[:n].view(pkg.HIT_DTYPE).reshape(-1), as_pkg_hits(pkg, ans["hits"][t]), "device trace")
    assert np.array_equal(occ[:m].astype(bool), ans["occ"]), "device occlusion"
    assert_same_floats(rgb[:n], ans["shoot"][(t, 5)], "device shoot")
    host_rgb, host_status = tracer.shade_hits(as_pkg_hits(pkg, ans["hits"][t]))
    same_bits(d_shade.cpu().numpy()[:n], host_rgb, "device shade_hits colours")
    assert np.array_equal(d_status.cpu().numpy()[:n], host_status)
